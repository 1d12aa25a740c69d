"""bench.py command-line surface (CPU-only): what --dump-outputs writes and
which options belong to the --full run."""
import pathlib
import sys

import numpy as np
import pytest

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import bench  # noqa: E402


def test_dump_outputs_formats(tmp_path):
    big = np.array([2 ** 63 + 12345, 7], dtype=np.uint64)  # not exact in f64
    neg = np.array([-(2 ** 60) - 1, 5], dtype=np.int64)    # not exact in f64
    outs = {
        "q1": {"returnflag": np.array([65, 78], np.uint8),
               "sum_qty": np.array([1.5, 2.25]),
               "count": np.array([3, 2 ** 40], np.int64),
               "sum_charge_lo": big,
               "neg": neg},
        "q5": {7: 12, 9: 2 ** 62 + 1},  # distributed q5: nation -> scalar
    }
    bench.dump_outputs(tmp_path / "d", outs)
    got = {p.name[:-4]: np.load(p) for p in (tmp_path / "d").glob("*.npy")}
    assert set(got) == {
        "q1.returnflag", "q1.sum_qty", "q1.count", "q1.sum_charge_lo",
        "q1.sum_charge_lo.hi32", "q1.sum_charge_lo.lo32", "q1.neg",
        "q1.neg.hi32", "q1.neg.lo32", "q5.7", "q5.9", "q5.9.hi32",
        "q5.9.lo32"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["q1.returnflag"].dtype == np.float32
    assert got["q1.returnflag"].tolist() == [65.0, 78.0]
    assert got["q1.sum_qty"].tolist() == [1.5, 2.25]
    assert got["q1.count"].tolist() == [3.0, float(2 ** 40)]
    assert got["q5.7"].tolist() == [12.0]
    # the halves put the exact 64-bit pattern back together
    for key, src in (("q1.sum_charge_lo", big), ("q1.neg", neg)):
        hi = got[key + ".hi32"].astype(np.int64)
        lo = got[key + ".lo32"].astype(np.int64)
        assert ((hi << 32) | lo).tolist() == src.view(np.int64).tolist()


def test_dump_outputs_samples_large_columns(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4096)
    col = np.arange(5000, dtype=np.float64)
    bench.dump_outputs(tmp_path / "a", {"q": {"x": col, "y": col[:3]}})
    bench.dump_outputs(tmp_path / "b", {"q": {"x": col, "y": col[:3]}})
    a, b = np.load(tmp_path / "a/q.x.npy"), np.load(tmp_path / "b/q.x.npy")
    assert 0 < a.size < col.size and np.array_equal(a, b)
    assert np.all(np.diff(a) > 0) and np.all(np.isin(a, col))
    assert np.load(tmp_path / "a/q.y.npy").tolist() == [0.0, 1.0, 2.0]
    total = sum(p.stat().st_size for p in (tmp_path / "a").iterdir())
    assert total <= 4096


def test_dump_outputs_rejects_missing_result(tmp_path):
    with pytest.raises(RuntimeError):
        bench.dump_outputs(tmp_path, {"q3": None})


def test_verify_needs_full(monkeypatch, capsys):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--verify"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2
    assert "--full" in capsys.readouterr().err
