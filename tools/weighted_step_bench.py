#!/usr/bin/env python3
"""Time of the fused training step of bench.py's headline workload (config 2, one GPU, eager launches) with and without class
weights: the same model, batch, optimiser arguments and timing scheme as ``python bench.py --gpus 1`` (warm-up, then regions of
K steps bracketed by a synchronisation), run alternately so both see the same machine state.

    python tools/weighted_step_bench.py [--steps 200] [--warmup 20] [--regions 5]

Prints one JSON line: ``ms_per_step`` of every region for ``unweighted`` and ``weighted`` (balanced weights of the batch's own
room labels through ``hmp_label_counts`` / ``hmp_balanced_class_weights``), and their medians."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "hydra-gnn_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--batch", type=int, default=None)
    a = ap.parse_args()
    import bench
    import hydra_gnn_amd.models as hmodels
    from hydra_gnn_amd import _lib

    argv, sys.argv = sys.argv, ["bench.py", "--gpus", "1"] + (["--batch", str(a.batch)] if a.batch else [])
    try:
        args = bench.parse()
    finally:
        sys.argv = argv
    dev = torch.device("cuda", 0)
    model_kw, cls_name, batch_cpu, label_type, workload = bench.make_workload(args, 0)
    batch = batch_cpu.to(dev)
    labels = batch[label_type].y
    lib = _lib.require_device()
    C = int(model_kw["output_dim"])
    counts = torch.zeros(C + 1, dtype=torch.int64, device=dev)
    weights = torch.empty(C, dtype=torch.float32, device=dev)
    _lib.check(lib.hmp_label_counts(labels.data_ptr(), labels.numel(), None, 25, C, counts.data_ptr(), _lib.stream_ptr()))
    _lib.check(lib.hmp_balanced_class_weights(counts.data_ptr(), C, weights.data_ptr(), _lib.stream_ptr()))

    steps = {}
    for name, w in (("unweighted", None), ("weighted", weights)):
        torch.manual_seed(1234)
        net = getattr(hmodels, cls_name)(**model_kw).to(dev)
        net.train()
        net.native().set_compute(args.precision)
        step = net.train_step(lr=0.002, weight_decay=0.001, ignored_label=25, seed=20250225, use_graph=False, class_weight=w)
        for _ in range(a.warmup):
            step(batch, labels)
        steps[name] = (net, step)
    ms = {name: [] for name in steps}
    for _ in range(a.regions):
        for name, (net, step) in steps.items():  # alternate: both forms see the same machine state
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step(batch, labels)
            torch.cuda.synchronize(dev)
            ms[name].append(1e3 * (time.perf_counter() - t0) / a.steps)
    out = {"workload": workload, "steps": a.steps, "warmup": a.warmup, "regions": a.regions}
    for name, (net, step) in steps.items():
        assert net.native().read_state() == (a.warmup + a.steps * a.regions, 0)
        out[name] = {"ms_per_step": [round(v, 5) for v in ms[name]], "median": round(float(np.median(ms[name])), 5),
                     "final_loss": step.loss()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
