"""bench.py's command line and its --dump-outputs writer (no GPU: the timed regions are not run)."""
import sys

import numpy as np
import pytest

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default_and_full_is_opt_in(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    a = _parse(monkeypatch, "--full", "--no-cpu-baseline", "--dump-outputs", "out")
    assert a.full and a.no_cpu_baseline and a.dump_outputs == "out"


@pytest.mark.parametrize("argv", [("--steps", "0"), ("--warmup", "-1")])
def test_step_counts_are_validated(monkeypatch, argv):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, *argv)


def test_dump_outputs_writes_float32_and_exact_float64(tmp_path):
    t = np.array([1.5, np.inf, 0.25], np.float32)             # the library's miss: +inf, id 0xFFFFFFFF
    ids = np.array([0, 0xFFFFFFFF, 99999], np.uint32)
    T = np.eye(4) * 1.0000000000000002
    bench.dump_outputs(str(tmp_path / "d"), {**bench.hit_outputs(t, ids), "icp_transformation": T, "icp_iterations": [20]})
    got = {p.stem: np.load(p) for p in (tmp_path / "d").glob("*.npy")}
    assert set(got) == {"t_hit", "primitive_ids", "icp_transformation", "icp_iterations"}
    assert all(np.isfinite(v).all() for v in got.values())
    assert got["t_hit"].dtype == np.float32 and got["t_hit"].tolist() == [1.5, -1.0, 0.25]
    assert got["primitive_ids"].dtype == np.float64 and np.array_equal(got["primitive_ids"].astype(np.uint32), ids)
    assert got["icp_transformation"].dtype == np.float64 and np.array_equal(got["icp_transformation"], T)
    assert got["icp_iterations"].tolist() == [20.0]


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_dump_outputs_refuses_non_finite_values(tmp_path, bad):
    with pytest.raises(RuntimeError):
        bench.dump_outputs(str(tmp_path / "d"), {"x": np.array([1.0, bad])})
    if not np.isposinf(bad):                                   # only +inf is a miss; NaN / -inf in t_hit stay errors
        with pytest.raises(RuntimeError):
            bench.dump_outputs(str(tmp_path / "d"), bench.hit_outputs(np.array([bad, np.inf], np.float32), [1, 2]))
    assert not (tmp_path / "d").exists()


def test_dump_outputs_refuses_more_than_64_mb(tmp_path):
    big = np.zeros(bench.DUMP_LIMIT_BYTES // 8 + 1, np.float64)
    with pytest.raises(RuntimeError):
        bench.dump_outputs(str(tmp_path / "d"), {"x": big})
    assert not (tmp_path / "d").exists()
