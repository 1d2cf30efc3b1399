"""CPU: the writer behind bench.py --dump-outputs (bench.dump_outputs): float32 files, the byte budget, whole arrays where
they fit, a seeded sample of rows for the rest, the same files every time."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_budget_and_sample(tmp_path, monkeypatch):
    bench = _bench_module()
    monkeypatch.setattr(bench, "DUMP_BYTES", 4 * 10000)
    g = torch.Generator().manual_seed(1)
    res = {"small": torch.rand(3, 4, generator=g), "mid": torch.rand(50, 3, generator=g, dtype=torch.float64),
           "big": torch.rand(4, 5000, 3, generator=g), "not_an_array": 7}
    bench.dump_outputs(res, str(tmp_path / "a"))
    bench.dump_outputs(res, str(tmp_path / "b"))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["big.npy", "mid.npy", "small.npy"] == sorted(os.listdir(tmp_path / "b"))
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    for f in files:
        assert got[f[:-4]].dtype == np.float32 and np.array_equal(got[f[:-4]], np.load(tmp_path / "b" / f))
    assert sum(a.size for a in got.values()) <= 10000
    assert np.array_equal(got["small"], res["small"].numpy()) and np.array_equal(got["mid"], res["mid"].float().numpy())
    # the large array: a sample of its xyz rows, each one a row of the array, in row order
    where = {tuple(r): i for i, r in enumerate(res["big"].reshape(-1, 3).numpy().tolist())}
    idx = [where[tuple(r)] for r in got["big"].tolist()]
    assert got["big"].shape[1] == 3 and 1000 < len(idx) < 20000 and idx == sorted(set(idx))
