"""Time one epoch of the two-headed (room + object) task, SemiSupervisedTrainingJob.train (semisupervised_training_job.py:113-160):
shuffled training batches, then one counting pass (val_mask) over the whole dataset -- two ways on one MI355X:

  host    data.collate / collate_homogeneous of the batch's graphs + .to(device) + step(batch, ...), then count_correct per
          host-collated batch (the DataLoader's work; only interfaces every commit with a fused two-head step has)
  stream  store.GraphStore + a two-headed BatchStream: stream.next(ids) + step.run(...), then count_correct on stream batches

on two stores:

  stanford  --graphs Stanford3DSG-like homogeneous graphs (workloads.stanford_like_graph, 2..27 nodes), HomogeneousNetwork
  mp3d      --graphs MP3D-like heterogeneous graphs (workloads.mp3d_like_graph), HeterogeneousNetwork

    python tools/semisup_epoch.py [--store stanford|mp3d|both] [--mode host|stream|both] [--graphs 384] [--batch-size 32]
                                  [--epochs 7] [--warmup 2]

Prints one JSON line per (store, mode): the epochs' wall times in ms, their median, minimum and spread (max - min), the last
loss and the val accuracy (equal between the modes: same seeds, same kernels).  Both modes draw the same permutations.  Under
`rocprofv3 --kernel-trace --stats -- python tools/semisup_epoch.py --mode stream --epochs 1 --warmup 0` collate_batch_kernel shows
one launch per batch (training and counting)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hydra-gnn_amd"))

from hydra_gnn_amd import workloads  # noqa: E402
from hydra_gnn_amd.data import collate, collate_homogeneous  # noqa: E402
from hydra_gnn_amd.models import HeterogeneousNetwork, HomogeneousNetwork  # noqa: E402

MASKS = ("train_mask", "val_mask", "test_mask")
LR, WD = 0.002, 0.001


def split(rng, n):
    u = torch.from_numpy(rng.random(n))
    return u < 0.6, (u >= 0.6) & (u < 0.8), u >= 0.8


def make_store(kind, n_graphs):
    """(graphs, model): the per-graph dataset with its masks, generated here so that every commit sees the same data"""
    rng = np.random.Generator(np.random.PCG64(workloads.BASE_SEED + (71 if kind == "stanford" else 72)))
    torch.manual_seed(0)
    if kind == "stanford":
        graphs = [workloads.stanford_like_graph(rng) for _ in range(n_graphs)]
        for g in graphs:
            g.train_mask, g.val_mask, g.test_mask = split(rng, g.num_nodes)
        model = HomogeneousNetwork(input_dim=6, output_dim_dict={"room": 15, "object": 35}, conv_block="GraphSAGE", hidden_dim=64,
                                   num_layers=3, dropout=0.25)
    else:
        graphs = [workloads.mp3d_like_graph(rng) for _ in range(n_graphs)]
        for g in graphs:
            for t in ("rooms", "objects"):
                g[t].train_mask, g[t].val_mask, g[t].test_mask = split(rng, int(g[t].y.numel()))
        model = HeterogeneousNetwork({"objects": 306, "rooms": 6}, output_dim_dict={"rooms": 26, "objects": 28},
                                     conv_block="GraphSAGE", hidden_dim=64, num_layers=3, dropout=0.25)
    return graphs, model


def run(kind, mode, args, dev):
    graphs, model = make_store(kind, args.graphs)
    model = model.to(dev).train()
    homog = kind == "stanford"
    step = model.semisupervised_step(lr=LR, weight_decay=WD, use_graph=False)
    n, bs = len(graphs), args.batch_size
    eval_ids = [list(range(i, min(i + bs, n))) for i in range(0, n, bs)]
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    if mode == "stream":
        from hydra_gnn_amd.store import GraphStore

        stream = GraphStore(graphs, dev).stream(model, bs)

    def host_batch(ids):
        sel = [graphs[j] for j in ids]
        return (collate_homogeneous(sel) if homog else collate(sel)).to(dev)

    def epoch(perm):
        for i in range(0, n, bs):
            ids = perm[i:i + bs]
            if mode == "stream":
                step.run(stream.next(ids), mask="train_mask")
            elif homog:
                step(host_batch(ids))
            else:
                b = host_batch(ids)
                step(b, (b["rooms"].y, b["objects"].y), (b["rooms"].train_mask, b["objects"].train_mask))
        counts.zero_()
        for ids in eval_ids:
            if mode == "stream":
                if homog:
                    model.count_correct(stream.next(ids), "val_mask", counts)
                else:
                    model.count_correct(stream.next(ids), None, "val_mask", counts)
            elif homog:
                model.count_correct(host_batch(ids), "val_mask", counts)
            else:
                b = host_batch(ids)
                model.count_correct(b, (b["rooms"].y, b["objects"].y), (b["rooms"].val_mask, b["objects"].val_mask), counts)
        return counts.cpu().tolist()  # the one synchronisation of the pass

    rng = np.random.Generator(np.random.PCG64(5))
    times, c = [], None
    for e in range(args.warmup + args.epochs):
        perm = rng.permutation(n)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        c = epoch(perm)
        dt = time.perf_counter() - t0
        if e >= args.warmup:
            times.append(1e3 * dt)
    res = {"store": kind, "mode": mode, "graphs": n, "batch_size": bs, "epochs_ms": [round(t, 3) for t in times],
           "median_ms": round(float(np.median(times)), 3), "min_ms": round(min(times), 3),
           "spread_ms": round(max(times) - min(times), 3), "last_loss": step.loss(),
           "val_accuracy": (c[0] + c[2]) / max(c[1] + c[3], 1)}
    print(json.dumps(res), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--store", default="both", choices=["stanford", "mp3d", "both"])
    ap.add_argument("--mode", default="both", choices=["host", "stream", "both"])
    ap.add_argument("--graphs", type=int, default=384)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for kind in (("stanford", "mp3d") if args.store == "both" else (args.store,)):
        for mode in (("host", "stream") if args.mode == "both" else (args.mode,)):
            run(kind, mode, args, dev)


if __name__ == "__main__":
    main()
