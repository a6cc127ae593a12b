"""ms per training step of the two-headed (room + object) task on config-2 (SAGE hidden 64, 3 layers, B = 32) and config-3 (GAT
128 x 4 heads, B = 64) shaped ``workloads.semisupervised_batch``es, timed with HIP events after warm-up:

* ``autograd``: the reference's loop body -- ``net(batch)`` -> ``net.loss`` -> ``backward`` -> ``torch.optim.Adam``;
* ``fused_eager`` / ``fused_graph``: ``semisupervised_step`` without / with hipGraph replay;
* ``single_graph``: the single-output fused step (``train_step``, room labels) of the same architecture on the same batch, the floor.

    python tools/semisup_step.py [--steps 100] [--warmup 20] [--out result.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "hydra-gnn_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from hydra_gnn_amd import workloads  # noqa: E402
from hydra_gnn_amd.models import HeterogeneousNetwork  # noqa: E402

DEV = "cuda:0"
SHAPES = {
    "config2_sage": (dict(conv_block="GraphSAGE", hidden_dim=64, num_layers=3, dropout=0.25), 32),
    "config3_gat": (dict(conv_block="GAT", GAT_hidden_dims=[128, 128], GAT_heads=[4, 4, 4], GAT_concats=[True, True, False],
                         dropout=0.25), 64),
}


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def measure(name, steps, warmup):
    kw, B = SHAPES[name]
    base = dict(input_dim_dict={"objects": 306, "rooms": 6}, **kw)
    gb = workloads.semisupervised_batch(B, workloads.BASE_SEED + 7).to(DEV)
    labels = (gb["rooms"].y, gb["objects"].y)
    masks = (gb["rooms"].train_mask, gb["objects"].train_mask)
    res = {"batch": B, "rows": {t: int(gb[t].y.numel()) for t in ("rooms", "objects")}}

    torch.manual_seed(0)
    net = HeterogeneousNetwork(output_dim_dict={"rooms": 26, "objects": 28}, **base).to(DEV).train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-4, weight_decay=1e-3)

    def autograd_step():
        opt.zero_grad()
        net.loss(net(gb), labels, masks).backward()
        opt.step()

    res["autograd"] = timed(autograd_step, steps, warmup)
    for use_graph, key in ((False, "fused_eager"), (True, "fused_graph")):
        step = net.semisupervised_step(lr=1e-4, weight_decay=1e-3, use_graph=use_graph)
        res[key] = timed(lambda: step(gb, labels, masks), steps, warmup)
    torch.manual_seed(0)
    one = HeterogeneousNetwork(output_dim=26, **base).to(DEV)
    s1 = one.train_step(lr=1e-4, weight_decay=1e-3, ignored_label=25, use_graph=True)
    yr = gb["rooms"].y
    res["single_graph"] = timed(lambda: s1(gb, yr), steps, warmup)
    res["speedup_graph_vs_autograd"] = res["autograd"] / res["fused_graph"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {name: measure(name, a.steps, a.warmup) for name in a.shapes.split(",")}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
