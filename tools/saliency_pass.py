"""Time the gradient-saliency calls on one MI355X, in one run: BASELINE config 2's room classifier (3-layer HeteroConv(GraphSAGE),
hidden 64) on one MP3D-like frame and on a 32-graph config-2 batch, each way beside `predict_labels` on the same input, so the
cost reads as a multiple of the eval forward.

    gradients   model.input_gradients(batch): eval forward + seed launch + the backward chain without the weight gradients
    saliency    model.saliency(batch): gradients + one reduction launch per node type
    labels      model.predict_labels(batch): the comparison -- the same forward and one launch
  results stay on the device; on the host:
    explain     model.explain_rooms(batch, k=3, by="gradient"): exact per-room passes (one per room ordinal of a graph), all
                queued without a synchronisation, one copy at the end
    confidence  model.predict_with_confidence(batch): its counterpart among the label calls

    python tools/saliency_pass.py [--graphs 32] [--repeats 5] [--calls 1000] [--gat] [--tag T]

Every repeat times `--calls` calls of each way in turn -- the ways alternate inside a repeat, so drift of the host hits them alike --
after one untimed round, and every timed window ends in a device synchronise (`explain` is timed over calls / 10 calls: it is
tens of passes).  One JSON line: per-repeat us per call, their medians and spreads (max - min), the pass counts of `explain`,
and `agree`: column 0 of `explain` is, for every room, the object with the largest |gradient x input| of a pass that selects
that room alone."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hydra-gnn_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hydra_gnn_amd import workloads  # noqa: E402
from hydra_gnn_amd.models import HeterogeneousNetwork  # noqa: E402
from topk_pass import summary, timed  # noqa: E402

O2R = ("objects", "objects_to_rooms", "rooms")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--gat", action="store_true")
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    kw = dict(input_dim_dict={"objects": 306, "rooms": 6}, output_dim=26, conv_block="GraphSAGE", hidden_dim=64, num_layers=3, dropout=0.25)
    if args.gat:
        kw = dict(input_dim_dict={"objects": 306, "rooms": 6}, output_dim=26, conv_block="GAT", GAT_hidden_dims=[128, 128],
                  GAT_heads=[4, 4, 4], GAT_concats=[True, True, False], dropout=0.25)
    model = HeterogeneousNetwork(**kw).to(dev).eval()
    batch = workloads.config2_batch(args.graphs).to(dev)
    frame = workloads.config2_batch(1).to(dev)

    def ways(b):
        return {"gradients": lambda: model.input_gradients(b), "saliency": lambda: model.saliency(b), "labels": lambda: model.predict_labels(b)}

    def host_ways(b):
        return {"explain": lambda: model.explain_rooms(b, k=3, by="gradient"), "confidence": lambda: model.predict_with_confidence(b)}

    few = max(args.calls // 10, 1)
    nat = model.native()
    out = {"tool": "saliency_pass", "tag": args.tag, "conv_block": kw["conv_block"], "graphs_per_batch": args.graphs,
           "repeats": args.repeats, "calls": args.calls, "host_calls": few,
           "frame_us": summary(timed(ways(frame), args.repeats, args.calls, 1e6)),
           "batch_us": summary(timed(ways(batch), args.repeats, args.calls, 1e6)),
           "frame_host_us": summary(timed(host_ways(frame), args.repeats, few, 1e6)),
           "batch_host_us": summary(timed(host_ways(batch), args.repeats, few, 1e6)),
           "frame_passes": nat.max_graph_rows(frame, "rooms"), "batch_passes": nat.max_graph_rows(batch, "rooms"),
           "frame_rooms": int(frame["rooms"].x.size(0)), "batch_rooms": int(batch["rooms"].x.size(0)),
           "frame_objects": int(frame["objects"].x.size(0)), "batch_objects": int(batch["objects"].x.size(0))}
    # column 0 of explain: the object with the largest |gradient x input| of the room's own pass
    agree = True
    src, sco = (t.clone() for t in model.explain_rooms(frame, k=3, by="gradient"))
    ei = frame[O2R].edge_index.cpu()
    for r in range(src.size(0)):
        rows = torch.zeros(src.size(0), dtype=torch.bool, device=dev)
        rows[r] = True
        gxi = model.saliency(frame, groups=(), rows=rows)["objects"][0].cpu()
        objs = torch.unique(ei[0][ei[1] == r])
        if objs.numel() == 0:
            agree = agree and int(src[r, 0]) == -1
            continue
        best = objs[torch.sort(gxi[objs].abs(), descending=True, stable=True).indices[0]]
        agree = agree and int(src[r, 0]) == int(best) and float(sco[r, 0]) == float(gxi[best])
    out["agree"] = bool(agree)
    assert nat.read_state()[1] == 0
    print(json.dumps(out))
    if not agree:
        sys.exit(1)


if __name__ == "__main__":
    main()
