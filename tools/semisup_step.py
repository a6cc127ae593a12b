"""ms per training step of the two-headed (room + object) task, timed with HIP events after warm-up, on

* config-2 (SAGE hidden 64, 3 layers, B = 32) and config-3 (GAT 128 x 4 heads, B = 64) shaped ``workloads.semisupervised_batch``es
  (``HeterogeneousNetwork``, heads = the program's own final states);
* the six homogeneous Stanford3DSG shapes of ``train_Stanford.py`` (B = 128, dropout 0.25, 15 room / 35 object classes, 6-d
  features; learned linear heads): ``HomogeneousNetwork`` on ``workloads.stanford_semisupervised_batch`` and
  ``HomogeneousNeuralTreeNetwork`` on H-tree batches from the committed fixture (built like
  tests/test_gpu_htree.py::homogeneous_htree_batch);
* the two heterogeneous H-tree Stanford3DSG shapes (``htree_hetero_GAT`` / ``htree_hetero_GAT_edge``: GAT hidden [64, 64, 64],
  heads 6, concats [T, T, T, F], no pre_mp, B = 128, 6-d features): ``HeterogeneousNeuralTreeNetwork`` on
  ``workloads.semisupervised_htree_batch``, each head's CE on the LeafPool of its final state:

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
from hydra_gnn_amd.models import (HeterogeneousNetwork, HeterogeneousNeuralTreeNetwork, HomogeneousNetwork,  # noqa: E402
                                   HomogeneousNeuralTreeNetwork)

DEV = "cuda:0"
SHAPES = {
    "config2_sage": (dict(conv_block="GraphSAGE", hidden_dim=64, num_layers=3, dropout=0.25), 32),
    "config3_gat": (dict(conv_block="GAT", GAT_hidden_dims=[128, 128], GAT_heads=[4, 4, 4], GAT_concats=[True, True, False],
                         dropout=0.25), 64),
}

_G6 = dict(GAT_hidden_dims=[128, 128], GAT_heads=[6, 6], GAT_concats=[True, True])
_G6x4 = dict(GAT_hidden_dims=[128] * 4, GAT_heads=[6] * 4, GAT_concats=[True] * 4)
STANFORD = {  # name: (H-tree, model kwargs)
    "baseline_GraphSAGE": (False, dict(conv_block="GraphSAGE", hidden_dim=128, num_layers=3)),
    "baseline_GAT": (False, dict(conv_block="GAT", **_G6)),
    "baseline_GAT_edge": (False, dict(conv_block="GAT_edge", **_G6)),
    "htree_GraphSAGE": (True, dict(conv_block="GraphSAGE", hidden_dim=128, num_layers=4)),
    "htree_GAT": (True, dict(conv_block="GAT", **_G6x4)),
    "htree_GAT_edge": (True, dict(conv_block="GAT_edge", **_G6x4)),
}
STANFORD_OUT = {"room": 15, "object": 35}
_G64 = dict(GAT_hidden_dims=[64, 64, 64], GAT_heads=[6, 6, 6, 6], GAT_concats=[True, True, True, False])
HETERO_HTREE = {  # config/Stanford3D/htree_hetero_GAT{,_edge}.yaml
    "htree_hetero_GAT": dict(conv_block="GAT", **_G64),
    "htree_hetero_GAT_edge": dict(conv_block="GAT_edge", **_G64),
}


def stanford_htree_batch(n_graphs, seed):
    """H-tree graphs of the committed fixture through the hetero -> homogeneous conversion, 6-d features, per-node labels (room
    classes on the room rows), seeded train split"""
    import numpy as np

    from hydra_gnn_amd.data import collate_homogeneous, heterogeneous_htree_to_homogeneous

    npz = np.load(workloads.HTREE_FIXTURE)
    rng = np.random.Generator(np.random.PCG64(seed))
    graphs = []
    for i in range(n_graphs):
        d = heterogeneous_htree_to_homogeneous(workloads.htree_graph(npz, i % int(npz["n_graphs"]), rng))
        del d.__dict__["edge_type"]
        graphs.append(d)
    b = collate_homogeneous(graphs)
    b.x = b.x[:, :6].contiguous()
    n = b.x.size(0)
    y = torch.from_numpy(rng.integers(0, 35, size=n))
    y[b.room_mask] = torch.from_numpy(rng.integers(0, 15, size=int(b.room_mask.sum())))
    b.y = y
    b.train_mask = torch.from_numpy(rng.random(n) < 0.6)
    return b


def measure_stanford(name, steps, warmup, n_graphs=128):
    htree, kw = STANFORD[name]
    seed = workloads.BASE_SEED + 7
    gb = stanford_htree_batch(n_graphs, seed) if htree else workloads.stanford_semisupervised_batch(n_graphs, seed)
    if kw["conv_block"] == "GAT_edge":  # relative positions of the endpoints
        gb.edge_attr = (gb.x[gb.edge_index[1], :3] - gb.x[gb.edge_index[0], :3]).contiguous()
    gb = gb.to(DEV)
    cls = HomogeneousNeuralTreeNetwork if htree else HomogeneousNetwork
    base = dict(input_dim=6, dropout=0.25, **kw)
    if htree:
        base.update(disable_initialization=True)
    res = {"batch": n_graphs, "rows": int(gb.x.size(0))}
    torch.manual_seed(0)
    net = cls(output_dim_dict=dict(STANFORD_OUT), **base).to(DEV).train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-4, weight_decay=1e-3)
    rm = gb.room_mask
    om = gb.object_mask if htree else ~rm
    labels, masks = (gb.y[rm], gb.y[om]), (gb.train_mask[rm], gb.train_mask[om])

    def autograd_step():
        opt.zero_grad()
        net.loss(net(gb), labels, masks).backward()
        opt.step()

    res["autograd"] = timed(autograd_step, steps, warmup)
    for use_graph, key in ((False, "fused_eager"), (True, "fused_graph")):
        step = net.semisupervised_step(lr=1e-4, weight_decay=1e-3, use_graph=use_graph)
        res[key] = timed(lambda: step(gb), steps, warmup)
    torch.manual_seed(0)
    if "GAT_hidden_dims" in base:  # single output: the last GAT layer maps to the classes (reference :73-77)
        base = dict(base, GAT_hidden_dims=base["GAT_hidden_dims"][:-1], GAT_concats=base["GAT_concats"][:-1] + [False])
    one = cls(output_dim=35, **base).to(DEV)
    s1 = one.train_step(lr=1e-4, weight_decay=1e-3, ignored_label=-100, use_graph=True)
    res["single_graph"] = timed(lambda: s1(gb, gb.y), steps, warmup)
    res["speedup_graph_vs_autograd"] = res["autograd"] / res["fused_graph"]
    return res


def measure_hetero_htree(name, steps, warmup, n_graphs=128):
    kw = HETERO_HTREE[name]
    gb = workloads.semisupervised_htree_batch(n_graphs, workloads.BASE_SEED + 7, relative_pos=kw["conv_block"] == "GAT_edge")
    for t in gb.node_types:  # 6-d features on every node type
        if "x" in gb[t]:
            gb[t].x = gb[t].x[:, :6].contiguous()
    gb = gb.to(DEV)
    dims = {t: 6 for t in ("object", "room", "object-room", "room-room", "object_virtual", "room_virtual")}
    base = dict(input_dim_dict=dims, dropout=0.25, disable_initialization=True, **kw)
    labels = (gb["room_virtual"].y, gb["object_virtual"].y)
    masks = (gb["room_virtual"].train_mask, gb["object_virtual"].train_mask)
    res = {"batch": n_graphs, "rows": {t: int(gb[t].num_nodes) for t in gb.node_types}}
    torch.manual_seed(0)
    out = dict(STANFORD_OUT, **{"object-room": 1, "room-room": 1})
    net = HeterogeneousNeuralTreeNetwork(output_dim_dict=out, **base).to(DEV).train()
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
    one = HeterogeneousNeuralTreeNetwork(output_dim=15, **base).to(DEV)
    s1 = one.train_step(lr=1e-4, weight_decay=1e-3, ignored_label=-100, use_graph=True)
    yr = gb["room_virtual"].y
    res["single_graph"] = timed(lambda: s1(gb, yr), steps, warmup)
    res["speedup_graph_vs_autograd"] = res["autograd"] / res["fused_graph"]
    return res


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
    ap.add_argument("--shapes", default=",".join(list(SHAPES) + list(STANFORD) + list(HETERO_HTREE)))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    def measure_any(name):
        if name in HETERO_HTREE:
            return measure_hetero_htree(name, a.steps, a.warmup)
        return (measure_stanford if name in STANFORD else measure)(name, a.steps, a.warmup)

    out = {name: measure_any(name) for name in a.shapes.split(",")}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
