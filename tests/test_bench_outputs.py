"""bench.py's options of a plain run: `--steps` sets the timed steps, the
line carries `ms_per_step`, `--full` is what adds the CPU baseline and the
per-kernel pass, and `--dump-outputs DIR` writes what the timed path returned
after its last timed step (float32 / float64 .npy files, 64 MB at most, a
larger X as a fixed seeded sample)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_small_output_is_written_whole(tmp_path):
    import bench
    X = np.arange(1000, dtype=np.float32)
    Dif = np.linspace(1, 0, 8).astype(np.float32)
    bench.dump_outputs(str(tmp_path / "o"), (X, 5, None, Dif), 0, 1)
    got = _load(str(tmp_path / "o"))
    assert sorted(got) == ["Dif", "X", "iterations"]
    assert got["X"].dtype == np.float32 and np.array_equal(got["X"], X)
    assert np.array_equal(got["Dif"], Dif[:5])
    assert got["iterations"].dtype == np.float64 and got["iterations"].tolist() == [5.0]


def test_dump_large_output_is_a_fixed_sample_within_64_MB(tmp_path):
    import bench
    n = bench.DUMP_BYTES // 4 + 12345  # one entry more than fits is enough; f32
    X = np.arange(n, dtype=np.float32) * 0.5
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), (X, 3, None, None), 0, 1)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sorted(a) == ["X", "X_index", "iterations"]
    assert all(np.array_equal(a[k], b[k]) for k in a)  # the same entries every run
    idx = a["X_index"].astype(np.int64)
    assert idx.size > 1000000 and idx.min() >= 0 and idx.max() < n
    assert np.array_equal(a["X"], X[idx])
    size = sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a")))
    assert size <= bench.DUMP_BYTES == 64 * 1000 * 1000
    # every rank of a partitioned run writes files of its own, within its share
    bench.dump_outputs(str(tmp_path / "r"), (X, 3, None, None), 1, 2)
    r = _load(str(tmp_path / "r"))
    assert sorted(r) == ["X_index_rank1", "X_rank1", "iterations_rank1"]
    assert sum(v.nbytes for v in r.values()) <= bench.DUMP_BYTES // 2


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_its_last_iterate(tmp_path):
    """one plain run of the 1.25M-vertex slab workload: 3 timed steps after 1
    warmup step; X.npy is the iterate after those 4 iterations, bit for bit
    what a session of its own gives on the same inputs"""
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload",
                        "headline_slab8", "--steps", "3", "--warmup", "1", "--dump-outputs", out],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    d = lines[0]
    assert d["steps"] == 3 and d["warmup"] == 1
    assert d["ms_per_step"] > 0 and d["unit"] == "Medge-updates/s" and d["dtype"] == "f32"
    assert d["higher_is_better"] is True and d["config"]["finite"] is True
    # value and ms_per_step state the same measurement
    E = d["config"]["E_per_gpu"]
    assert d["value"] == pytest.approx(E / d["ms_per_step"] / 1e3, rel=1e-3)
    # nothing that takes a run of its own without --full
    assert d["cpu_baseline"] is None and d["roofline"]["kernels"] == {}
    got = _load(out)
    assert sorted(got) == ["X", "iterations"]
    assert got["iterations"].tolist() == [4.0]
    from cp_pfdr_graph_d1_amd import pfdr
    from workloads import WORKLOADS
    wl = WORKLOADS["headline_slab8"]
    inp = wl.inputs(0, 1)
    sess = pfdr.Session(wl.kind, wl.dtype, inp["V"], inp["E"], itMax=4, **inp["kw"])
    assert sess.run(4) == 4
    X = sess.result()[0]
    sess.close()
    assert got["X"].dtype == np.float32 and got["X"].shape == X.shape
    assert np.all(np.isfinite(X)) and np.any(X != 0)
    assert np.array_equal(got["X"], X)
