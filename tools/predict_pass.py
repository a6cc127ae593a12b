"""Time one label-export pass over a device-resident dataset on one MI355X, three ways:

  a  evaluate.predict(model, (stream, id_lists)): every batch collated on the device, predict_labels into its slice of one buffer,
     ONE device-to-host copy per pass
  b  room task: a loop of model.predict(batch) over batches collated beforehand (native forward + argmax, one D2H per batch)
  c  two-headed task: [p.argmax(1).cpu() for p in model(batch)] per batch (the reference's spelling, two D2H per batch)

    python tools/predict_pass.py --task room   [--batches 64] [--graphs 32] [--repeats 5] [--passes 20] [--only ab]
    python tools/predict_pass.py --task two    [--n 384]      [--graphs 32] [--repeats 5] [--passes 20] [--only ac]

`room`: the 64 x 32-graph MP3D-like validation pass of tools/eval_pass.py (config 2's HeteroConv(SAGE) room classifier).  `two`: the
384-graph Stanford-like store of the two-headed task (HomogeneousNetwork GraphSAGE with two linear heads), batches of 32.

b and c only use interfaces older trees have, so the same file times them there (`--only b` / `--only c`).  Every repeat times
`--passes` passes after one untimed pass and ends in a device synchronise; one JSON line per run with the per-repeat ms per pass,
their median and spread (max - min).  With a and another way selected, the labels of both are compared and must be equal."""
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
from hydra_gnn_amd.data import collate, collate_homogeneous  # noqa: E402
from hydra_gnn_amd.models import HeterogeneousNetwork, HomogeneousNetwork  # noqa: E402
from hydra_gnn_amd.store import GraphStore  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", choices=("room", "two"), default="room")
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--n", type=int, default=384)
    ap.add_argument("--graphs", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--only", default=None)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    only = args.only or ("ab" if args.task == "room" else "ac")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    if args.task == "room":
        model = HeterogeneousNetwork({"objects": 306, "rooms": 6}, output_dim=26, conv_block="GraphSAGE", hidden_dim=64, num_layers=3,
                                     dropout=0.25).to(dev).eval()
        rng = np.random.Generator(np.random.PCG64(workloads.BASE_SEED + 91))
        graphs = [workloads.mp3d_like_graph(rng) for _ in range(args.batches * args.graphs)]
        coll, stream_kw = collate, dict(label_type="rooms")
    else:
        model = HomogeneousNetwork(input_dim=6, output_dim_dict={"room": 15, "object": 35}, conv_block="GraphSAGE", hidden_dim=64,
                                   num_layers=3, dropout=0.25).to(dev).eval()
        graphs = workloads.stanford_semisupervised_graphs(args.n, workloads.BASE_SEED + 92)
        coll, stream_kw = collate_homogeneous, {}
    n = len(graphs)
    ids = [list(range(i, min(i + args.graphs, n))) for i in range(0, n, args.graphs)]
    loader = [coll([graphs[j] for j in b]).to(dev) for b in ids]
    store = GraphStore(graphs, dev)
    stream = store.stream(model, args.graphs, **stream_kw)

    def way_a():
        from hydra_gnn_amd import evaluate

        return evaluate.predict(model, (stream, ids))  # per graph

    def way_b():
        return [model.predict(b).clone() for b in loader]  # per batch

    def way_c():
        with torch.no_grad():
            return [[p.argmax(1).cpu() for p in model(b)] for b in loader]  # per batch, (room rows, object rows)

    ways = {"a": way_a, "b": way_b, "c": way_c}
    out = {"tool": "predict_pass", "tag": args.tag, "task": args.task, "graphs": n, "graphs_per_batch": args.graphs,
           "batches": len(ids), "repeats": args.repeats, "passes": args.passes, "ms_per_pass": {}, "median": {}, "spread": {}}
    results = {}
    for k in only:
        fn = ways[k]
        results[k] = fn()  # untimed: workspace, plans, pinned buffers
        runs = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.passes):
                fn()
            torch.cuda.synchronize()
            runs.append(1e3 * (time.perf_counter() - t0) / args.passes)
        out["ms_per_pass"][k] = [round(v, 4) for v in runs]
        out["median"][k] = round(statistics.median(runs), 4)
        out["spread"][k] = round(max(runs) - min(runs), 4)
    if "a" in results and len(results) > 1:  # the same labels, graph by graph
        per_graph = results["a"]
        other = results.get("b", results.get("c"))
        flat = []
        if args.task == "room":
            rooms = [int(g["rooms"].num_nodes) for g in graphs]
            for b, lab in zip(ids, other):
                off = np.concatenate([[0], np.cumsum([rooms[j] for j in b])])
                flat.extend(lab.numpy()[off[i]:off[i + 1]] for i in range(len(b)))
            out["agree"] = all(np.array_equal(x, y) for x, y in zip(per_graph, flat))
        else:
            got = [np.concatenate([g[h] for g in per_graph]) for h in range(2)]
            want = [np.concatenate([lab[h].numpy() for lab in other]) for h in range(2)]
            # forward() computes the heads on the matrix pipe, predict on the VALU: near-ties may differ
            out["differing_rows"] = [int((x != y).sum()) for x, y in zip(got, want)]
            out["agree"] = sum(out["differing_rows"]) * 100 <= sum(x.size for x in got)
    assert model.native().read_state()[1] == 0
    stream.close()
    print(json.dumps(out))
    if out.get("agree") is False:
        sys.exit(1)


if __name__ == "__main__":
    main()
