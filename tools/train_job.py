"""Time the epoch loop of a training job two ways on one MI355X:

  hand  the loop in the reference's shape written with the public pieces every commit has: step.run(stream.next(ids)), then
        `step.loss()` per step (a D2H read), evaluate.accuracy / semisupervised_accuracy per epoch (a D2H read) and
        deepcopy(net.state_dict()) on every strict improvement
  job   hydra_gnn_amd.jobs: BaseTrainingJob.train / SemiSupervisedTrainingJob.train (bookkeeping on the device, csrc/epoch.hip);
        the module is imported in this mode only, so `--mode hand` runs on commits that do not have it

on three shapes:

  room  MP3D-like room task at config-2 shapes: 384 train / 96 val / 32 test graphs, batch 32, 3 x HeteroConv(SAGE), hidden 64
  semi  the Stanford-like two-headed task of tools/semisup_epoch.py: 384 homogeneous graphs, batch 32, GraphSAGE, hidden 64
  homog_room  (job mode only) the room task on Stanford-like homogeneous graphs, BASELINE config 1's model family: 384 train / 96
        val / 32 test graphs, batch 32, GraphSAGE, hidden 64; followed by one line for `job.test_individual_graph` on 64 graphs
        (ms per call, `--repeats` calls after one untimed call)

    python tools/train_job.py [--mode hand|job|both] [--shape room|semi|homog_room|both] [--epochs 50] [--warmup 5] [--repeats 5]

Each repeat trains `warmup` epochs untimed, then times `epochs` epochs (wall clock around the loop, device synchronised at both
ends).  One JSON line per (shape, mode): ms per epoch of every repeat, their median, minimum and spread.  Under
`rocprofv3 --kernel-trace --stats -- python tools/train_job.py --mode job --repeats 1` the epoch_* kernels show their own times.
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hydra-gnn_amd"))

from hydra_gnn_amd import evaluate, workloads  # noqa: E402
from hydra_gnn_amd.store import GraphStore  # noqa: E402

LR, WD, B = 0.002, 0.001, 32
ROOM_PARAMS = dict(conv_block="GraphSAGE", hidden_dim=64, num_layers=3, dropout=0.25)


def room_graphs():
    rng = np.random.Generator(np.random.PCG64(workloads.BASE_SEED + 81))
    gs = [workloads.mp3d_like_graph(rng) for _ in range(384 + 96 + 32)]
    return {"train": gs[:384], "val": gs[384:480], "test": gs[480:]}


def semi_graphs():
    rng = np.random.Generator(np.random.PCG64(workloads.BASE_SEED + 71))
    gs = [workloads.stanford_like_graph(rng) for _ in range(384)]
    for g in gs:
        u = torch.from_numpy(rng.random(g.num_nodes))
        g.train_mask, g.val_mask, g.test_mask = u < 0.6, (u >= 0.6) & (u < 0.8), u >= 0.8
    return gs


def homog_room_graphs():
    """Stanford-like graphs (one room each) whose room label follows the room's size feature, three of the 15 classes: random labels
    can leave every validation room wrong, and a run without an improvement has no best state"""
    rng = np.random.Generator(np.random.PCG64(workloads.BASE_SEED + 91))
    gs = [workloads.stanford_like_graph(rng) for _ in range(384 + 96 + 32)]
    for g in gs:
        g.y[0] = min(int((float(g.x[0, 3]) - 0.1) / 2.9 * 3), 2)
    return {"train": gs[:384], "val": gs[384:480], "test": gs[480:]}


def chunks(n):
    return [list(range(i, min(i + B, n))) for i in range(0, n, B)]


def hand_loop(shape, args, dev):
    """ms per epoch of the hand loop"""
    from torch.utils.data import DataLoader

    from hydra_gnn_amd.models import HeterogeneousNetwork, HomogeneousNetwork

    torch.manual_seed(0)
    if shape == "room":
        split = room_graphs()
        net = HeterogeneousNetwork({"objects": 306, "rooms": 6}, output_dim=26, **ROOM_PARAMS).to(dev)
        streams = {s: GraphStore(g, dev).stream(net, B, "rooms") for s, g in split.items()}
        step = net.train_step(lr=LR, weight_decay=WD, ignored_label=25, use_graph=False)
        n_train = len(split["train"])
        valid = [int((g["rooms"].y != 25).sum()) for g in split["train"]]

        def train_batch(ids):
            step.run(streams["train"].next(ids))
            return step.loss(), sum(valid[i] for i in ids)

        val = lambda: evaluate.accuracy(net, (streams["val"], chunks(len(split["val"]))))
        loss_div = None
    else:
        gs = semi_graphs()
        net = HomogeneousNetwork(input_dim=6, output_dim_dict={"room": 15, "object": 35}, **ROOM_PARAMS).to(dev)
        stream = GraphStore(gs, dev).stream(net, B)
        step = net.semisupervised_step(lr=LR, weight_decay=WD, use_graph=False)
        n_train = len(gs)

        def train_batch(ids):
            step.run(stream.next(ids), mask="train_mask")
            return step.loss(), len(ids)

        val = lambda: evaluate.semisupervised_accuracy(net, (stream, chunks(n_train)), "val_mask")
        loss_div = n_train
    loader = DataLoader(range(n_train), batch_size=B, shuffle=True)
    state = {"max": 0, "best": None}

    def epoch():
        total, weights = 0.0, 0
        net.train()
        for ids in loader:
            loss, w = train_batch(ids.tolist())
            total += loss * w
            weights += w
        total /= loss_div if loss_div is not None else weights
        net.eval()
        v = val()
        if v > state["max"]:
            state["max"], state["best"] = v, copy.deepcopy(net.state_dict())
        return total

    times = []
    for _ in range(args.repeats):
        for _ in range(args.warmup):
            epoch()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.epochs):
            epoch()
        torch.cuda.synchronize(dev)
        times.append(1e3 * (time.perf_counter() - t0) / args.epochs)
    return times


class _Info:
    def __init__(self, features, rooms, objects=None):
        self._f, self._r, self._o = features, rooms, objects

    def num_node_features(self):
        return self._f

    def num_room_labels(self):
        return self._r

    def num_object_labels(self):
        return self._o


class _Dataset:
    def __init__(self, data_type, graphs, info):
        self._type, self._graphs, self._info = data_type, graphs, info

    def data_type(self):
        return self._type

    def __len__(self):
        return len(self._graphs)

    def __getitem__(self, i):
        return self._graphs[i]

    def get_data(self, i):
        return self._info


def job_loop(shape, args, dev):
    """ms per epoch of job.train (its own `training_time`: the loop, the restore of the best state and the one read)"""
    from hydra_gnn_amd import jobs

    torch.manual_seed(0)
    params = {k: v for k, v in ROOM_PARAMS.items()}
    if shape == "room":
        info = _Info({"objects": 306, "rooms": 6}, 26)
        job = jobs.BaseTrainingJob({s: _Dataset("heterogeneous", g, info) for s, g in room_graphs().items()}, params)
    elif shape == "homog_room":
        split = homog_room_graphs()
        job = jobs.BaseTrainingJob({s: _Dataset("homogeneous", g, _Info(6, 15)) for s, g in split.items()}, params)
    else:
        job = jobs.SemiSupervisedTrainingJob(_Dataset("homogeneous", semi_graphs(), _Info(6, 15, 35)), params)
    opt = {"lr": LR, "weight_decay": WD, "batch_size": B, "shuffle": True}
    times = []
    with tempfile.TemporaryDirectory() as log_folder:
        for _ in range(args.repeats):
            job.train(log_folder, dict(opt, num_epochs=max(args.warmup, 1)))
            _, _, info = job.train(log_folder, dict(opt, num_epochs=args.epochs))
            times.append(1e3 * info["training_time"] / info["num_epochs"])
    if shape == "homog_room":
        dataset = _Dataset("homogeneous", (split["val"] + split["test"])[:64], _Info(6, 15))
        job.test_individual_graph(dataset)
        calls = []
        for _ in range(args.repeats):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            job.test_individual_graph(dataset)
            calls.append(1e3 * (time.perf_counter() - t0))
        print(json.dumps({"shape": shape, "what": "test_individual_graph", "graphs": len(dataset), "batch_size": B,
                          "ms_per_call": [round(t, 3) for t in calls], "median_ms": round(float(np.median(calls)), 3),
                          "min_ms": round(min(calls), 3), "spread_ms": round(max(calls) - min(calls), 3)}), flush=True)
    return times


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="both", choices=["hand", "job", "both"])
    ap.add_argument("--shape", default="both", choices=["room", "semi", "homog_room", "both"])
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for shape in (("room", "semi") if args.shape == "both" else (args.shape,)):
        for mode in (("hand", "job") if args.mode == "both" and shape != "homog_room" else ("job",) if shape == "homog_room" else (args.mode,)):
            times = (hand_loop if mode == "hand" else job_loop)(shape, args, dev)
            print(json.dumps({"shape": shape, "mode": mode, "epochs": args.epochs, "batch_size": B,
                              "ms_per_epoch": [round(t, 3) for t in times], "median_ms": round(float(np.median(times)), 3),
                              "min_ms": round(min(times), 3), "spread_ms": round(max(times) - min(times), 3)}), flush=True)


if __name__ == "__main__":
    main()
