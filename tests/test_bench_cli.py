"""CPU: bench.py's command line and its --dump-outputs writer (no GPU needed)."""
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _results(n_atoms, n_frames, seed=3):
    rng = np.random.RandomState(seed)
    return {"energy": rng.rand(n_frames), "forces": rng.rand(n_atoms, 3),
            "virial": rng.rand(n_frames, 3, 3), "atomic": rng.rand(n_atoms)}


def test_dump_outputs_writes_every_array_in_float64(tmp_path):
    res = _results(40, 2)
    meta = bench.dump_outputs(str(tmp_path / "out"), res)
    assert meta["atom_sample"] is None
    for k, v in res.items():
        a = np.load(str(tmp_path / "out" / (k + ".npy")))
        assert a.dtype == np.float64
        np.testing.assert_array_equal(a, v)


def test_dump_outputs_samples_atoms_under_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096)
    res = _results(1000, 3)
    m1 = bench.dump_outputs(str(tmp_path / "a"), res)
    m2 = bench.dump_outputs(str(tmp_path / "b"), res)
    assert m1["bytes"] <= 4096 and m1 == {**m2, "dir": m1["dir"]}
    keep = m1["atom_sample"]["atoms_kept"]
    assert 0 < keep < 1000
    f = np.load(str(tmp_path / "a" / "forces.npy"))
    e = np.load(str(tmp_path / "a" / "atomic.npy"))
    assert f.shape == (keep, 3) and e.shape == (keep,)
    np.testing.assert_array_equal(f, np.load(str(tmp_path / "b" / "forces.npy")))
    # the same atoms in both per-atom arrays, in the order of the batch
    rows = [int(np.flatnonzero((res["forces"] == r).all(axis=1))[0]) for r in f]
    assert rows == sorted(rows)
    np.testing.assert_array_equal(e, res["atomic"][rows])
    np.testing.assert_array_equal(np.load(str(tmp_path / "a" / "virial.npy")), res["virial"])


def test_bench_refuses_zero_steps():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "--steps" in p.stderr
