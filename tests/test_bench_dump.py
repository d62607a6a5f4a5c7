"""bench.py's --dump-outputs writer: whole arrays under the byte budget, a fixed seeded row
sample over it, per-rank names with more than one rank."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_whole_array_under_budget(tmp_path):
  x = np.random.default_rng(1).normal(size=(37, 27))
  bench.dump_outputs(str(tmp_path / "d"), {"qfrc_inverse": x})
  assert sorted(os.listdir(tmp_path / "d")) == ["qfrc_inverse.npy"]
  y = np.load(tmp_path / "d" / "qfrc_inverse.npy")
  assert y.dtype == np.float64
  np.testing.assert_array_equal(y, x)


def test_seeded_sample_over_budget(tmp_path, monkeypatch):
  monkeypatch.setattr(bench, "DUMP_BYTES", 4096)
  x = np.random.default_rng(2).normal(size=(301, 5)).astype(np.float32)
  for d in ("a", "b"):
    bench.dump_outputs(str(tmp_path / d), {"u": x, "v": 2 * x}, world=2, rank=1)
  names = sorted(os.listdir(tmp_path / "a"))
  assert names == ["u_rank1.npy", "u_rank1_rows.npy", "v_rank1.npy", "v_rank1_rows.npy"]
  # both ranks' files together stay within the budget
  assert 2 * sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 4096 + 2 * 4 * 128
  rows = np.load(tmp_path / "a" / "u_rank1_rows.npy")
  assert rows.dtype == np.float64 and (np.diff(rows) > 0).all() and 0 < len(rows) < 301
  u = np.load(tmp_path / "a" / "u_rank1.npy")
  assert u.dtype == np.float32
  np.testing.assert_array_equal(u, x[rows.astype(int)])
  for n in names:       # the same rows and values from run to run
    np.testing.assert_array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n))


def test_rejects_other_dtypes(tmp_path):
  with pytest.raises(AssertionError):
    bench.dump_outputs(str(tmp_path), {"i": np.arange(4)})
