"""`bench.py --steps K --dump-outputs DIR` on the GPU: exactly K timed steps, and the outputs of the last one written as .npy files
that two runs with the same arguments reproduce exactly (seeded inputs, deterministic engine)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--no-cpu-baseline", "--no-roofline", "--dump-outputs", out_dir],
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip())


@pytest.mark.gpu
def test_bench_dump_outputs_two_runs_agree(tmp_path):
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    outs = [_bench(d) for d in dirs]
    for out in outs:
        assert out["steps"] == 7 and out["timed_steps_total"] == 7 and out["timed_regions"] == 1
        assert out["ms_per_step"] > 0
    names = sorted(f for f in os.listdir(dirs[0]))
    assert names == ["adam_m.npy", "adam_v.npy", "loss.npy", "params.npy"]
    assert sum(os.path.getsize(os.path.join(dirs[0], f)) for f in names) <= 64 << 20
    for f in names:
        a, b = np.load(os.path.join(dirs[0], f)), np.load(os.path.join(dirs[1], f))
        assert a.dtype in (np.float32, np.float64) and a.size > 0 and np.isfinite(a).all(), f
        np.testing.assert_array_equal(a, b, err_msg=f)
    assert 0.0 < float(np.load(os.path.join(dirs[0], "loss.npy"))[0]) < 10.0
    assert outs[0]["dump_outputs"]["arrays"]["params"][0] == outs[0]["dump_outputs"]["arrays"]["params"][1]  # no sampling
