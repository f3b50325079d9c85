"""bench.py --dump-outputs: the sample of a large result is fixed (two builds dump the same
elements), ascending, in bounds, holds both ends, and stays far below the 64 MB a dump may take;
a small result is dumped whole.  --full and --dump-outputs are options of the command line.  CPU."""
from __future__ import annotations

import importlib.util
import pathlib
import subprocess
import sys

import numpy as np

REPO = pathlib.Path(__file__).resolve().parents[1]


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", REPO / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_sample_index_is_fixed_and_bounded():
    b = _bench()
    n, k = (1 << 28), (1 << 22)
    i1, i2 = b.sample_index(n, k), b.sample_index(n, k)
    assert i1.dtype == np.int64 and np.array_equal(i1, i2)
    assert i1.size == k + 2 * b.DUMP_EDGE and i1.size * 4 <= 64 << 20
    assert i1[0] == 0 and i1[-1] == n - 1 and np.all(np.diff(i1) >= 0)
    assert np.array_equal(i1[:b.DUMP_EDGE], np.arange(b.DUMP_EDGE))
    assert np.array_equal(i1[-b.DUMP_EDGE:], np.arange(n - b.DUMP_EDGE, n))


def test_sample_index_small_result_whole():
    b = _bench()
    assert np.array_equal(b.sample_index(1000, 1 << 22), np.arange(1000))


def test_dump_output_writes_float32_npy(tmp_path):
    import torch
    b = _bench()
    n = 4 * b.DUMP_EDGE
    t = torch.arange(n, dtype=torch.float64)
    b.dump_output(torch, str(tmp_path / "d"), "x", t, 16)
    got = np.load(tmp_path / "d" / "x.npy")
    assert got.dtype == np.float32 and got.shape == (16 + 2 * b.DUMP_EDGE,)
    assert np.array_equal(got, b.sample_index(n, 16).astype(np.float32))  # t[i] = i


def test_command_line_has_full_and_dump_outputs():
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout
