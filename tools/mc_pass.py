"""Time Monte-Carlo dropout uncertainty on one MI355X, in one run: `predict_mc(samples)` against the torch route built from public
pieces, on two passes over collated batches.

  mp3d      the MP3D-like validation pass of tools/predict_pass.py (config 2's HeteroConv(SAGE) room classifier, 26 classes)
  stanford  a Stanford-like pass of the two-headed homogeneous GraphSAGE model (15 room / 35 object classes, learned linear heads)

  mc        model.predict_mc(batch, samples) per batch: per sample the native training-mode forward plus one launch, one finishing
            launch per head; the five arrays of every head and batch concatenated on the device and copied once per pass
  torch     per batch and sample the training-mode model(batch) at the dropout step predict_mc draws at, softmax, entropy and the
            running sums in torch, the statistics from the sums; the same five arrays concatenated and copied once per pass

    python tools/mc_pass.py [--samples 16] [--batches 16] [--graphs 32] [--repeats 5] [--passes 5] [--tag T]

The torch route needs nothing this tool's commit adds: on a commit without `predict_mc` the tool times that route alone.  Every
repeat times `--passes` passes of each way in turn -- the ways alternate inside a repeat -- after one untimed round, and every timed
window ends in a device synchronise.  One JSON line: per-repeat ms per pass, their medians and spreads (max - min), and how far the two
routes' mean probabilities lie apart (`max_mean_diff`; labels are compared on the rows whose top-two gap of the torch mean exceeds
4e-5)."""
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


def timed(ways, repeats, count):
    """per way: [ms per pass] per repeat, the ways alternating inside every repeat; one untimed round first"""
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
            runs[name].append(1e3 * (time.perf_counter() - t0) / count)
    return runs


def summary(runs):
    return {"runs": {k: [round(v, 4) for v in r] for k, r in runs.items()},
            "median": {k: round(statistics.median(r), 4) for k, r in runs.items()},
            "spread": {k: round(max(r) - min(r), 4) for k, r in runs.items()}}


def down(heads_per_batch):
    """every array of every head and batch as float32 in one device buffer, one copy; returns the host pieces in order"""
    flat = [t for heads in heads_per_batch for hd in heads for t in hd]
    host = torch.cat([t.reshape(-1).to(torch.float32) for t in flat]).cpu().numpy()
    sizes = np.cumsum([0] + [t.numel() for t in flat])
    return [host[sizes[i]:sizes[i + 1]].reshape(tuple(t.shape)) for i, t in enumerate(flat)]


def torch_route(model, batches, T):
    """(labels, mean_probs, std, entropy, mutual_info) per head and batch from T training-mode forwards, all in torch"""
    was, step = model.training, model._rng_step
    model.train()
    out = []
    with torch.no_grad():
        for b in batches:
            model._rng_step = 0  # forward() draws at step 1, 2, ...: predict_mc's first_step = 1
            sums = None
            for _ in range(T):
                logits = model(b)
                logits = logits if isinstance(logits, tuple) else (logits,)
                ps = [torch.softmax(x, 1) for x in logits]
                hs = [-(p * torch.log(p.clamp_min(1e-38))).sum(1) for p in ps]
                if sums is None:
                    sums = [[p.clone(), p * p, h] for p, h in zip(ps, hs)]
                else:
                    for s, p, h in zip(sums, ps, hs):
                        s[0] += p
                        s[1] += p * p
                        s[2] += h
            heads = []
            for A, B, E in sums:
                mean = A / T
                lab = mean.argmax(1)
                best = mean.gather(1, lab[:, None])[:, 0]
                sd = (B.gather(1, lab[:, None])[:, 0] / T - best * best).clamp_min(0).sqrt()
                ent = -(mean * torch.log(mean.clamp_min(1e-38))).sum(1)
                heads.append((lab, mean, sd, ent, (ent - E / T).clamp_min(0)))
            out.append(heads)
    model._rng_step = step
    model.train(was)
    return down(out)


def mc_route(model, batches, T, rows_of):
    out = []
    for b in batches:
        res = model.predict_mc(b, samples=T)
        heads = list(res) if isinstance(res[0], tuple) else [res]
        out.append([tuple(t[m] for t in hd) if m is not None else hd for hd, m in zip(heads, rows_of(b, len(heads)))])
    return down(out)


def compare(a, b):
    """the two routes' host pieces: largest |mean difference| and whether the labels agree off the near-ties"""
    worst, agree, rows, used = 0.0, True, 0, 0
    for i in range(0, len(a), 5):
        mean_t = b[i + 1].astype(np.float64)
        worst = max(worst, float(np.abs(a[i + 1] - b[i + 1]).max()) if mean_t.size else 0.0)
        if mean_t.shape[1] >= 2:
            top = np.sort(mean_t, axis=1)[:, ::-1]
            clear = top[:, 0] - top[:, 1] > 4e-5
        else:
            clear = np.ones(mean_t.shape[0], dtype=bool)
        agree = agree and bool(np.array_equal(a[i][clear], b[i][clear]))
        rows, used = rows + clear.size, used + int(clear.sum())
    return worst, agree, rows, used


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--graphs", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    T = args.samples
    torch.manual_seed(0)
    n = args.batches * args.graphs
    chunks = [list(range(i, i + args.graphs)) for i in range(0, n, args.graphs)]
    rng = np.random.Generator(np.random.PCG64(workloads.BASE_SEED + 91))
    mp3d = HeterogeneousNetwork({"objects": 306, "rooms": 6}, output_dim=26, conv_block="GraphSAGE", hidden_dim=64, num_layers=3,
                                dropout=0.25).to(dev).eval()
    graphs = [workloads.mp3d_like_graph(rng) for _ in range(n)]
    mp3d_batches = [collate([graphs[j] for j in c]).to(dev) for c in chunks]
    stanford = HomogeneousNetwork(input_dim=6, output_dim_dict={"room": 15, "object": 35}, conv_block="GraphSAGE", hidden_dim=64,
                                  num_layers=3, dropout=0.25).to(dev).eval()
    sgraphs = workloads.stanford_semisupervised_graphs(n, workloads.BASE_SEED + 92)
    stanford_batches = [collate_homogeneous([sgraphs[j] for j in c]).to(dev) for c in chunks]
    whole = lambda b, heads: [None] * heads  # noqa: E731
    node_rows = lambda b, heads: [b.room_mask, ~b.room_mask]  # noqa: E731  (forward() returns the heads' rows compacted)
    out = {"tool": "mc_pass", "tag": args.tag, "samples": T, "graphs": n, "graphs_per_batch": args.graphs, "batches": len(chunks),
           "repeats": args.repeats, "passes": args.passes}
    have = hasattr(mp3d, "predict_mc")
    for name, model, batches, rows_of in (("mp3d", mp3d, mp3d_batches, whole), ("stanford", stanford, stanford_batches, node_rows)):
        ways = {"torch": lambda: torch_route(model, batches, T)}
        if have:
            ways["mc"] = lambda: mc_route(model, batches, T, rows_of)
        out[name + "_ms"] = summary(timed(ways, args.repeats, args.passes))
        if have:
            worst, agree, rows, used = compare(mc_route(model, batches, T, rows_of), torch_route(model, batches, T))
            out[name] = {"rows": rows, "rows_compared": used, "agree": agree, "max_mean_diff": worst}
        assert model.native().read_state()[1] == 0
    print(json.dumps(out))
    if have and not (out["mp3d"]["agree"] and out["stanford"]["agree"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
