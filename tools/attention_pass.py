"""Time the attention export on one MI355X, in one run: BASELINE config 3's room classifier (3-layer HeteroConv(GAT, 4 heads), hidden
128) on one MP3D-like frame and on a 32-graph config-3 batch, each four ways -- all of them "eval forward + 1 launch", results left
on the device, plus the host form for the frame.

    attention   model.attention(batch): alpha of every live conv of the last layer (three edge types into the rooms)
    top3        model.top_attended(batch, ("objects", "objects_to_rooms", "rooms"), k=3)
    labels      model.predict_labels(batch): the comparison -- the same forward and one launch
  frame only
    explain     model.explain_rooms(frame, k=3): top3 on the host through one pinned buffer and one copy
    confidence  model.predict_with_confidence(frame): its counterpart among the label calls

    python tools/attention_pass.py [--graphs 32] [--repeats 5] [--calls 2000] [--gat-edge] [--tag T]

Every repeat times `--calls` calls of each way in turn -- the ways alternate inside a repeat, so drift of the host hits them alike --
after one untimed round, and every timed window ends in a device synchronise.  One JSON line: per-repeat us per call, their
medians and spreads (max - min).  The head-mean top-3 of `top3` is compared with the order of the exported alpha (`agree`)."""
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
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--gat-edge", action="store_true")
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    kw = dict(input_dim_dict={"objects": 306, "rooms": 6}, output_dim=26, conv_block="GAT", GAT_hidden_dims=[128, 128],
              GAT_heads=[4, 4, 4], GAT_concats=[True, True, False], dropout=0.25)
    if args.gat_edge:
        kw.update(input_dim_dict={"objects": 303, "rooms": 3}, conv_block="GAT_edge")
    model = HeterogeneousNetwork(**kw).to(dev).eval()
    batch = workloads.config3_batch(args.graphs, edge=args.gat_edge).to(dev)
    frame = workloads.config3_batch(1, edge=args.gat_edge).to(dev)

    def ways(b):
        return {"attention": lambda: model.attention(b), "top3": lambda: model.top_attended(b, O2R, k=3),
                "labels": lambda: model.predict_labels(b)}

    frame_ways = dict(ways(frame), explain=lambda: model.explain_rooms(frame, k=3), confidence=lambda: model.predict_with_confidence(frame))
    out = {"tool": "attention_pass", "tag": args.tag, "conv_block": kw["conv_block"], "graphs_per_batch": args.graphs,
           "repeats": args.repeats, "calls": args.calls,
           "frame_us": summary(timed(frame_ways, args.repeats, args.calls, 1e6)),
           "batch_us": summary(timed(ways(batch), args.repeats, args.calls, 1e6))}
    # top3 is the stable descending order of the exported alpha's head means
    alpha = model.attention(batch)[O2R].cpu()
    src, w = (t.cpu() for t in model.top_attended(batch, O2R, k=3))
    ei = batch[O2R].edge_index.cpu()
    mean = alpha[:, 0]
    for h in range(1, alpha.size(1)):
        mean = mean + alpha[:, h]
    mean = mean / alpha.size(1)
    agree = True
    for r in range(src.size(0)):
        e = torch.nonzero(ei[1] == r).flatten()
        order = torch.sort(mean[e], descending=True, stable=True).indices[:3]
        agree = agree and torch.equal(src[r, :order.numel()], ei[0][e][order]) and torch.equal(w[r, :order.numel()], mean[e][order])
    out["rooms"] = int(src.size(0))
    out["edges"] = int(ei.size(1))
    out["agree"] = bool(agree)
    assert model.native().read_state()[1] == 0
    print(json.dumps(out))
    if not agree:
        sys.exit(1)


if __name__ == "__main__":
    main()
