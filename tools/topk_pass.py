"""Time top-k labels with softmax confidence on one MI355X, in one run: a label-export pass over a device-resident dataset and a
single frame, each four ways.

  pass (the 64 x 32-graph MP3D-like validation pass of tools/predict_pass.py, config 2's HeteroConv(SAGE) room classifier)
    k1, k3   evaluate.predict_topk(model, (stream, id_lists), k) at k = 1 and k = 3: every batch collated on the device, eval
             forward + one launch into its slice of one buffer, ONE device-to-host copy per pass
    labels   evaluate.predict(model, (stream, id_lists)): the same pass with predict_labels
    torch    softmax(model(batch), 1).topk(3) over batches collated beforehand, the pieces concatenated on the device and copied
             once per pass (the route that existed before; it needs the logits as a tensor, which the room task has)
  frame (one MP3D-like scene graph, results on the host)
    k1       model.predict_with_confidence(frame): one pinned buffer, one copy
    k3       model.predict_topk(frame, 3), both outputs copied to the host
    labels   model.predict(frame)
    torch    softmax(model(frame), 1).topk(3), both outputs copied to the host

    python tools/topk_pass.py [--batches 64] [--graphs 32] [--repeats 5] [--passes 20] [--calls 2000] [--tag T]

Every repeat times `--passes` passes (`--calls` frame calls) of each way in turn -- the ways alternate inside a repeat, so drift of
the host hits them alike -- after one untimed round, and every timed window ends in a device synchronise.  One JSON line: per-repeat
ms per pass and us per call, their medians and spreads (max - min).  The top-3 labels of k3 are compared with torch's on every row
whose top four probabilities are distinct (`agree`)."""
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

from hydra_gnn_amd import evaluate, workloads  # noqa: E402
from hydra_gnn_amd.data import collate  # noqa: E402
from hydra_gnn_amd.models import HeterogeneousNetwork  # noqa: E402
from hydra_gnn_amd.store import GraphStore  # noqa: E402


def timed(ways, repeats, count, scale):
    """per way: [scale * seconds per call] per repeat, the ways alternating inside every repeat; one untimed round first"""
    for fn in ways.values():
        fn()
    runs = {name: [] for name in ways}
    for _ in range(repeats):
        for name, fn in ways.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(count):
                fn()
            torch.cuda.synchronize()
            runs[name].append(scale * (time.perf_counter() - t0) / count)
    return runs


def summary(runs):
    return {"runs": {k: [round(v, 4) for v in r] for k, r in runs.items()},
            "median": {k: round(statistics.median(r), 4) for k, r in runs.items()},
            "spread": {k: round(max(r) - min(r), 4) for k, r in runs.items()}}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--graphs", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = HeterogeneousNetwork({"objects": 306, "rooms": 6}, output_dim=26, conv_block="GraphSAGE", hidden_dim=64, num_layers=3,
                                 dropout=0.25).to(dev).eval()
    rng = np.random.Generator(np.random.PCG64(workloads.BASE_SEED + 91))
    graphs = [workloads.mp3d_like_graph(rng) for _ in range(args.batches * args.graphs)]
    n = len(graphs)
    ids = [list(range(i, min(i + args.graphs, n))) for i in range(0, n, args.graphs)]
    loader = [collate([graphs[j] for j in b]).to(dev) for b in ids]
    store = GraphStore(graphs, dev)
    stream = store.stream(model, args.graphs, label_type="rooms")
    frame = collate([graphs[0]]).to(dev)

    def torch_pass():
        with torch.no_grad():
            tops = [torch.softmax(model(b), 1).topk(3) for b in loader]
            return torch.cat([t.indices for t in tops]).cpu(), torch.cat([t.values for t in tops]).cpu()

    def torch_frame():
        with torch.no_grad():
            top = torch.softmax(model(frame), 1).topk(3)
            return top.indices.cpu(), top.values.cpu()

    def k3_frame():
        lab, prb = model.predict_topk(frame, 3)
        return lab.cpu(), prb.cpu()

    pass_ways = {"k1": lambda: evaluate.predict_topk(model, (stream, ids), 1), "k3": lambda: evaluate.predict_topk(model, (stream, ids), 3),
                 "labels": lambda: evaluate.predict(model, (stream, ids)), "torch": torch_pass}
    frame_ways = {"k1": lambda: model.predict_with_confidence(frame), "k3": k3_frame, "labels": lambda: model.predict(frame),
                  "torch": torch_frame}
    out = {"tool": "topk_pass", "tag": args.tag, "graphs": n, "graphs_per_batch": args.graphs, "batches": len(ids),
           "repeats": args.repeats, "passes": args.passes, "calls": args.calls,
           "pass_ms": summary(timed(pass_ways, args.repeats, args.passes, 1e3)),
           "frame_us": summary(timed(frame_ways, args.repeats, args.calls, 1e6))}
    # the same top-3 labels wherever torch's own order is not a matter of its tie-breaking
    got = evaluate.predict_topk(model, (stream, ids), 3)
    lab = np.concatenate([g[0] for g in got])
    prb = np.concatenate([g[1] for g in got])
    t_lab, t_prb = (t.numpy() for t in torch_pass())
    with torch.no_grad():
        full = torch.cat([torch.softmax(model(b), 1).topk(4).values for b in loader]).cpu().numpy()
    clear = (np.diff(full, axis=1) < 0).all(axis=1)
    out["rows"] = int(lab.shape[0])
    out["rows_compared"] = int(clear.sum())
    out["agree"] = bool(np.array_equal(lab[clear], t_lab[clear]))
    out["max_prob_diff"] = float(np.abs(prb - t_prb)[clear].max()) if clear.any() else 0.0
    assert model.native().read_state()[1] == 0
    stream.close()
    print(json.dumps(out))
    if not out["agree"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
