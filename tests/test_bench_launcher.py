"""bench.py --gpus N without a launcher around it starts its N ranks itself (how the driver calls it); CPU only: the ranks meet over
gloo and report what they saw (--launcher-selftest), no GPU is touched.  Also bench.py's own options: --steps, --dump-outputs, and (on the GPU)
what a run without --full prints and writes."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def test_gpus_n_launches_n_ranks_itself():
    r = _run(["--gpus", "2", "--launcher-selftest"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                               # rank 0's line only
    assert lines[0]["n_gpus"] == 2 and lines[0]["ranks_seen"] == 2 and lines[0]["world_size"] == 2


def test_gpus_must_match_the_launcher():
    r = _run(["--gpus", "3", "--launcher-selftest"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2 and "WORLD_SIZE=2" in r.stderr


def test_steps_below_one_is_refused():
    r = _run(["--steps", "0"])
    assert r.returncode == 2 and "--steps" in r.stderr


def test_dump_outputs_writes_the_tables_as_float_arrays(tmp_path):
    """--dump-outputs: the last timed step's (species_rows, strain_rows, stats) as float64 .npy files; names -> their numbers; every value
    finite: None -> 0.0 with its bit clear in the option bits, an unsolved LP's objective -> 0.0 with lp_objective_set 0."""
    import numpy as np
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from bench import dump_outputs
    out = ([("1000", 0.75, 12.5), ("1002", 0.25, 4.0)],
           [("1000", "GCF_000001003.1", 11.0, 0.6, 0.9, None, 2.0, 0.3, None, 1.5), ("1002", "GCF_000003000.1", 4.0, 0.4, 0.8, 0.5, None, 1.0, 0.1, 0.2)],
           dict(obj=[(1.0, 2.0), (float("nan"), float("nan")), (3.0, 4.0)], iters=[(1, 2), (0, 0), (3, 4)], n_rows=[5, 0, 6], n_cand=[2, 0, 3],
                n_patterns=[1, 0, 2], n_active=2))
    nbytes = dump_outputs(str(tmp_path / "d"), out)
    a = {f[:-4]: np.load(str(tmp_path / "d" / f)) for f in os.listdir(str(tmp_path / "d"))}
    assert sorted(a) == ["lp_candidates", "lp_iterations", "lp_objective", "lp_objective_set", "lp_patterns", "lp_rows", "species_table", "strain_table"]
    assert all(v.dtype == np.float64 and np.isfinite(v).all() for v in a.values()) and nbytes == sum(v.nbytes for v in a.values())
    assert a["species_table"].tolist() == [[1000.0, 0.75, 12.5], [1002.0, 0.25, 4.0]]
    st = a["strain_table"]
    assert st.shape == (2, 11) and st[:, :4].tolist() == [[1000.0, 10031.0, 11.0, 0.6], [1002.0, 30001.0, 4.0, 0.4]]
    assert st[:, 4].tolist() == [1 + 4 + 8 + 32, 1 + 2 + 8 + 16 + 32]
    assert st[0, 5:].tolist() == [0.9, 0.0, 2.0, 0.3, 0.0, 1.5] and st[1, 5:].tolist() == [0.8, 0.5, 0.0, 1.0, 0.1, 0.2]
    assert a["lp_objective"].tolist() == [[1.0, 2.0], [0.0, 0.0], [3.0, 4.0]] and a["lp_objective_set"].tolist() == [[1, 1], [0, 0], [1, 1]]
    assert a["lp_rows"].tolist() == [5.0, 0.0, 6.0]
    empty = dump_outputs(str(tmp_path / "e"), ([], [], dict(obj=[], iters=[], n_rows=[], n_cand=[], n_patterns=[])))
    assert empty == 0 and np.load(str(tmp_path / "e" / "strain_table.npy")).shape == (0, 11)
    with pytest.raises(ValueError, match="species_table"):
        dump_outputs(str(tmp_path / "f"), ([("1000", float("nan"), 1.0)], [], dict(obj=[], iters=[], n_rows=[], n_cand=[], n_patterns=[])))


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    """A run without --full: the line carries the headline keys only, --steps sets the timed steps, and --dump-outputs writes the tables of the
    last timed step -- the same arrays from a second run with another number of steps (the inputs are a function of the arguments)."""
    import numpy as np
    lines, dumps = [], []
    for k, steps in enumerate((3, 2)):
        d = tmp_path / ("d%d" % k)
        r = _run(["--gpus", "1", "--workload", "cfg2", "--steps", str(steps), "--warmup", "2", "--dump-outputs", str(d)], timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert line["steps"] == steps and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["full"] is False
        assert line["unit"] == "Mreads/s" and line["higher_is_better"] is True and line["dtype"] == "int64+f64"
        assert line["value"] == pytest.approx(1e6 / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-9)
        assert "cpu_baseline" not in line and "roofline" not in line and "detail_file" not in line
        lines.append(line)
        dumps.append({f: np.load(str(d / f)) for f in sorted(os.listdir(str(d)))})
    one, two = lines
    sp, st = dumps[0]["species_table.npy"], dumps[0]["strain_table.npy"]
    assert sp.dtype == np.float64 and len(sp) == one["result"]["n_species_rows"] > 0 and st.shape == (one["result"]["n_strain_rows"], 11)
    assert all(np.isfinite(v).all() for v in dumps[0].values())
    for row, (s, h, cov, ab) in zip(st, one["result"]["top_strains"]):
        assert row[0] == int(s) and row[2] == pytest.approx(cov, abs=1e-4) and row[3] == pytest.approx(ab, abs=1e-6)
    assert one["result"] == two["result"] and sorted(dumps[0]) == sorted(dumps[1])
    for f in dumps[0]:
        assert np.array_equal(dumps[0][f], dumps[1][f], equal_nan=True), f
