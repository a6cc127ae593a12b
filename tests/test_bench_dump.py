"""`bench.py --dump-outputs DIR`: what the timed step hands its caller, written as DIR/<name>.npy (CPU: a stand-in model and step;
the real run is tests/test_gpu_bench_dump.py)."""
import os

import numpy as np
import torch

import bench  # the repository root is on sys.path (tests/conftest.py)


class _Native:
    def __init__(self, offsets):
        self.param_offsets = offsets


class _Model(torch.nn.Module):
    """two parameters the executor owns (the second 16-byte aligned in its flat buffer, as engine.NativeNet lays them out) and
    one it does not"""

    def __init__(self, n):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(n, 3))
        self.b = torch.nn.Parameter(torch.zeros(5))
        self.unused = torch.nn.Parameter(torch.zeros(2))
        self._nat = _Native({id(self.w): 0, id(self.b): (3 * n + 3) // 4 * 4})

    def native(self):
        return self._nat


class _Step:
    def __init__(self, n):
        flat = torch.arange((3 * n + 3) // 4 * 4 + 8, dtype=torch.float32)
        self.flat, self.m, self.v = flat, 2 * flat, 3 * flat

    def loss(self):
        return 1.25


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_loss_params_and_moments_in_parameter_order(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    n = 7
    written = bench.dump_outputs(str(tmp_path), _Model(n), _Step(n))
    got = _load(str(tmp_path))
    assert sorted(got) == ["adam_m", "adam_v", "loss", "params"]
    want = np.concatenate([np.arange(3 * n), 24 + np.arange(5)]).astype(np.float32)  # the alignment gap is not an output
    np.testing.assert_array_equal(got["params"], want)
    np.testing.assert_array_equal(got["adam_m"], 2 * want)
    np.testing.assert_array_equal(got["adam_v"], 3 * want)
    assert got["loss"].dtype == np.float64 and got["loss"].tolist() == [1.25]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert written["params"] == [3 * n + 5, 3 * n + 5]


def test_dump_over_budget_is_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 64 << 10)
    n = 20000
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    for d in dirs:
        written = bench.dump_outputs(d, _Model(n), _Step(n))
    assert sum(os.path.getsize(os.path.join(dirs[0], f)) for f in os.listdir(dirs[0])) <= 64 << 10
    assert 0 < written["params"][0] < written["params"][1] == 3 * n + 5
    a, b = _load(dirs[0]), _load(dirs[1])
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    p = a["params"]
    assert np.all(np.diff(p) > 0)  # ascending element order, drawn from the whole array
    np.testing.assert_array_equal(a["adam_m"], 2 * p)
