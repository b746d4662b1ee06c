"""bench.py's options around the timed steps (CPU): --full is off by default and gates the legs that take runs of
their own; --dump-outputs writes the last step's arrays as float32 / float64 .npy files within the size budget,
large arrays as the same seeded sample from run to run."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_full_is_off_by_default():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not a.full and a.dump_outputs is None and (a.steps, a.warmup) == (7, 2)
    assert bench.parse(["--full"]).full
    assert bench.parse(["--dump-outputs", "d"]).dump_outputs == "d"


def test_gemm_calls_needs_full():
    with pytest.raises(SystemExit):
        bench.parse(["--gemm-calls", "calls.jsonl"])
    assert bench.parse(["--full", "--gemm-calls", "calls.jsonl"]).gemm_calls == "calls.jsonl"


def test_dump_outputs_small_arrays_whole(tmp_path):
    g = torch.Generator().manual_seed(1)
    arrays = {"a": torch.randn(5, 3, generator=g), "views": [torch.randn(4, 4, 3, generator=g) for _ in range(2)],
              "h": torch.randn(7, generator=g).half(), "loss": torch.tensor([0.25, 0.5], dtype=torch.float64),
              "absent": None}
    bench.dump_outputs(str(tmp_path / "o"), arrays)
    assert sorted(os.listdir(tmp_path / "o")) == ["a.npy", "h.npy", "loss.npy", "views.npy"]
    a, v, h, loss = (np.load(tmp_path / "o" / f"{k}.npy") for k in ("a", "views", "h", "loss"))
    assert a.dtype == np.float32 and np.array_equal(a, arrays["a"].numpy())
    assert v.shape == (2, 4, 4, 3) and np.array_equal(v[1], arrays["views"][1].numpy())
    assert h.dtype == np.float32 and np.array_equal(h, arrays["h"].float().numpy())
    assert loss.dtype == np.float64 and loss.tolist() == [0.25, 0.5]


def test_dump_outputs_samples_large_arrays_reproducibly(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4000)  # two files: 2000 bytes = 500 float32 each
    big = torch.arange(3000, dtype=torch.float32).reshape(30, 100)
    small = torch.arange(10, dtype=torch.float32)
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    x, y = np.load(tmp_path / "x" / "big.npy"), np.load(tmp_path / "y" / "big.npy")
    assert x.shape == (500,) and np.array_equal(x, y)
    assert np.all(np.diff(x) > 0) and x.max() > 2500  # distinct elements in index order, drawn from the whole array
    assert np.array_equal(np.load(tmp_path / "x" / "small.npy"), small.numpy())
    total = sum(os.path.getsize(tmp_path / "x" / f) for f in os.listdir(tmp_path / "x"))
    assert total <= 4000 + 2 * 128  # payload within the budget (+ the .npy headers)
