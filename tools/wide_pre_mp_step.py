"""Time one fused training step of the homogeneous H-tree room classifier on the full 306-d features on one MI355X, with the
`pre_mp` initialisation (a one-head 306 -> 306 GAT over `init_edge_index`: the GAT kernels' two-slices-per-lane class) on and off:

    python tools/wide_pre_mp_step.py [--graphs 32] [--repeats 5] [--steps 200] [--only on,off] [--block GraphSAGE]

Both models step on the SAME collated batch of `--graphs` H-tree graphs (the topology fixture, as the tests build them).  Every
repeat times `--steps` steps after untimed warm-up steps and ends in a device synchronise; the two variants alternate repeat by
repeat.  One JSON line: per-repeat ms per step, their median and spread (max - min) per variant, nodes and init edges of the
batch.  For the per-kernel split run it under `rocprofv3 --kernel-trace --stats` with `--only on`."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hydra-gnn_amd"))

from hydra_gnn_amd import workloads  # noqa: E402
from hydra_gnn_amd.data import collate_homogeneous, heterogeneous_htree_to_homogeneous  # noqa: E402
from hydra_gnn_amd.models import HomogeneousNeuralTreeNetwork  # noqa: E402

IGNORED = 25


def htree_batch(n_graphs: int, seed: int):
    npz = np.load(workloads.HTREE_FIXTURE)
    rng = np.random.Generator(np.random.PCG64(seed))
    k = int(npz["n_graphs"])
    graphs = []
    for i in range(n_graphs):
        d = heterogeneous_htree_to_homogeneous(workloads.htree_graph(npz, i % k, rng))
        del d.__dict__["edge_type"]
        graphs.append(d)
    return collate_homogeneous(graphs)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", default="on,off")
    ap.add_argument("--block", default="GraphSAGE")
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    batch = htree_batch(args.graphs, workloads.BASE_SEED + 93).to(dev)
    labels = torch.where(batch.room_mask, batch.y, torch.full_like(batch.y, IGNORED))
    steps = {}
    for which in args.only.split(","):
        torch.manual_seed(0)
        net = HomogeneousNeuralTreeNetwork(306, output_dim=26, conv_block=args.block, hidden_dim=args.hidden, num_layers=3,
                                           GAT_hidden_dims=[args.hidden] * 2, GAT_heads=[2, 2, 2], GAT_concats=[True, True, False],
                                           disable_initialization=(which == "off"), dropout=0.25).to(dev)
        step = net.train_step(lr=0.002, weight_decay=0.001, ignored_label=IGNORED, use_graph=False)
        for _ in range(args.warmup):
            step(batch, labels)
        torch.cuda.synchronize()
        steps[which] = (net, step)
    out = {"tool": "wide_pre_mp_step", "tag": args.tag, "block": args.block, "hidden": args.hidden, "graphs": args.graphs,
           "nodes": int(batch.x.size(0)), "edges": int(batch.edge_index.size(1)), "init_edges": int(batch.init_edge_index.size(1)),
           "repeats": args.repeats, "steps": args.steps, "ms_per_step": {k: [] for k in steps}, "median": {}, "spread": {}, "loss": {}}
    for _ in range(args.repeats):
        for which, (net, step) in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(batch, labels)
            torch.cuda.synchronize()
            out["ms_per_step"][which].append(round(1e3 * (time.perf_counter() - t0) / args.steps, 4))
    for which, (net, step) in steps.items():
        runs = out["ms_per_step"][which]
        out["median"][which] = round(statistics.median(runs), 4)
        out["spread"][which] = round(max(runs) - min(runs), 4)
        out["loss"][which] = step.loss()
        assert net.native().read_state()[1] == 0 and np.isfinite(out["loss"][which])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
