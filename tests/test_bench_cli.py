"""bench.py's command line: a plain run is the headline alone (--full off by
default) and --dump-outputs writes the caller's view of the last timed
evaluation as float64 .npy files. CPU only: nothing here starts the benchmark."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _parse(monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_full_is_off_by_default(monkeypatch):
    a = _parse(monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 3)
    a = _parse(monkeypatch, ["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_files(tmp_path):
    rows = np.array([5, 0, 9999, -1], dtype=np.int32)
    out = tmp_path / "new" / "dir"
    bench.dump_outputs(str(out), 0, 1, rows, 3, 1, 4)
    assert sorted(os.listdir(out)) == ["rows.npy", "totals.npy"]
    r, t = np.load(out / "rows.npy"), np.load(out / "totals.npy")
    assert r.dtype == np.float64 and t.dtype == np.float64
    assert r.tolist() == [5.0, 0.0, 9999.0, -1.0] and t.tolist() == [3.0, 1.0, 4.0]
    # one pair of files per rank when several ranks run
    bench.dump_outputs(str(out), 1, 2, rows, 3, 1, 4)
    assert "rows_rank1.npy" in os.listdir(out) and "totals_rank1.npy" in os.listdir(out)
