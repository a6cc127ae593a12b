"""Time one validation pass of the room task (BaseTrainingJob.test, base_training_job.py:269-313) four ways on one MI355X:

  a  the reference's shape: model(batch).argmax(dim=1), mask, pred.eq(label).sum().item() per batch
  b  model.predict(batch) (native forward + hmp_argmax_rows, one D2H per batch), labels compared on the host
  c  model.count_correct_rooms(batch, counts) on device batches (collated beforehand), one sync per pass
  d  store.BatchStream + count_correct_rooms: every batch collated on the device from the resident dataset, one sync per pass

    python tools/eval_pass.py [--batches 64] [--graphs 32] [--passes 5] [--only d]

Prints one JSON line: ms per pass (best of --passes) and the accuracy each way computed (they must agree).  Under
`rocprofv3 --kernel-trace --stats -- python tools/eval_pass.py --only cd --passes 1` every batch of c / d shows one
count_rows_kernel launch beyond the eval forward."""
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
from hydra_gnn_amd.data import collate  # noqa: E402
from hydra_gnn_amd.models import HeterogeneousNetwork  # noqa: E402
from hydra_gnn_amd.store import GraphStore  # noqa: E402

IGNORED = 25


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--graphs", type=int, default=32)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--only", default="abcd")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    # config 2's model: HeteroConv(SAGE), hidden 64, 3 layers, 26 room classes
    model = HeterogeneousNetwork({"objects": 306, "rooms": 6}, output_dim=26, conv_block="GraphSAGE", hidden_dim=64, num_layers=3,
                                 dropout=0.25).to(dev).eval()
    rng = np.random.Generator(np.random.PCG64(workloads.BASE_SEED + 91))
    n_graphs = args.batches * args.graphs
    graphs = [workloads.mp3d_like_graph(rng) for _ in range(n_graphs)]
    ids = [list(range(i * args.graphs, (i + 1) * args.graphs)) for i in range(args.batches)]
    loader = [collate([graphs[j] for j in b]).to(dev) for b in ids]
    host_labels = [b["rooms"].y.cpu() for b in loader]
    store = GraphStore(graphs, dev)
    stream = store.stream(model, args.graphs, "rooms")

    def way_a():
        correct = total = 0
        with torch.no_grad():
            for b in loader:
                pred = model(b).argmax(dim=1)
                label = b["rooms"].y
                mask = label != IGNORED
                correct += pred[mask].eq(label[mask]).sum().item()
                total += torch.numel(label[mask])
        return correct / total

    def way_b():
        correct = total = 0
        for b, label in zip(loader, host_labels):
            pred = model.predict(b)
            mask = label != IGNORED
            correct += int(pred[mask].eq(label[mask]).sum())
            total += int(mask.sum())
        return correct / total

    def way_c():
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        for b in loader:
            model.count_correct_rooms(b, counts)
        c, t = counts.tolist()
        return c / t

    def way_d():
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        for b in ids:
            model.count_correct_rooms(stream.next(b), counts)
        c, t = counts.tolist()
        return c / t

    ways = {"a": way_a, "b": way_b, "c": way_c, "d": way_d}
    out = {"batches": args.batches, "graphs_per_batch": args.graphs, "passes": args.passes, "ms_per_pass": {}, "accuracy": {}}
    for k in args.only:
        fn = ways[k]
        out["accuracy"][k] = fn()  # warm-up pass (workspace, plans)
        best = float("inf")
        for _ in range(args.passes):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        out["ms_per_pass"][k] = round(1e3 * best, 3)
    accs = set(out["accuracy"].values())
    out["agree"] = len(accs) == 1
    assert model.native().read_state()[1] == 0
    stream.close()
    print(json.dumps(out))
    if not out["agree"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
