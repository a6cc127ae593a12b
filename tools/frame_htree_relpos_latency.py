"""Latency of the H-tree frame conversion with relative positions on its edges (``FramePipeline(htree=True,
htree_relative_pos=True)``) next to what it is measured against:

  * ``pipeline_htree``: the same frame with ``htree=True`` alone (what the 17 extra items cost; also runs on a tree that does not
    have the new keyword yet, where the legs below are skipped),
  * ``python_typed``: the Python path a user would otherwise write -- ``RoomObjectGraph`` + ``object_connectivity`` +
    ``to_hetero_data`` + ``htree.generate_htree(clique_pos=True)`` + ``data.compute_relative_pos`` -- and ``python_homogeneous``: that
    plus one round trip through ``data.heterogeneous_htree_to_homogeneous`` on the host,
  * ``pipeline_htree_relpos`` / ``pipeline_htree_relpos_homogeneous``: the new mode, typed and homogeneous.

Every figure is the median and p90 of ``--reps`` calls (default 200) after 8 warm-ups, each call timed to completion (host call +
``torch.cuda.synchronize()``), the legs in alternation ``--rounds`` times (default 2).  Frames: the reference's test graph
(tests/golden, 62 kept objects, 5 rooms) and ``workloads.synthetic_scene(60, 3, seed=1)``.  Prints one JSON line per leg and round.
``--convert-loop N`` runs only N converts of the new mode per layout and frame, for a kernel trace.  ``--tree PATH`` takes the package
from another checkout (run from the repository root)."""
import argparse
import inspect
import json
import os
import sys
import time

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--convert-loop", type=int, default=0)
ap.add_argument("--tree", default=".")
ap.add_argument("--tag", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.join(args.tree, "hydra-gnn_amd"))
from hydra_gnn_amd import data as hdata, dsg, htree, workloads  # noqa: E402

DEV = "cuda:0"
CLIQUE_DIM = 6
FIXTURE = os.path.join("tests", "golden", "dsg_x8F5xyUWy9e.json")
HAS_MODE = "htree_relative_pos" in inspect.signature(dsg.FramePipeline.__init__).parameters


def scene_graph(arrays):
    ids, layer, pos, bb_min, bb_max, label, edges = arrays
    index = {int(v): i for i, v in enumerate(ids)}
    adj = [set() for _ in ids]
    for a, b in zip(edges[0].tolist(), edges[1].tolist()):
        a, b = index.get(a), index.get(b)
        if a is None or b is None or a == b:
            continue
        adj[a].add(b)
        adj[b].add(a)
    return dsg.SceneGraph(np.asarray(ids, dtype=np.uint64), np.asarray(layer, dtype=np.int64), np.asarray(pos, dtype=np.float64),
                          np.asarray(bb_min, dtype=np.float64), np.asarray(bb_max, dtype=np.float64), np.asarray(label, dtype=np.int64), adj)


def timed(fn, reps):
    for _ in range(8):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter_ns()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter_ns() - t0) * 1e-3)
    ts = np.array(ts)
    return {"median_us": round(float(np.median(ts)), 1), "p90_us": round(float(np.percentile(ts, 90)), 1)}


def main():
    frames = {"fixture": dsg.scene_arrays(dsg.load_dsg_json(FIXTURE)), "synthetic_60x3": workloads.synthetic_scene(60, 3, seed=1)}
    for name, arrays in frames.items():
        sg = scene_graph(arrays)
        legs = {}
        plain = dsg.FramePipeline(DEV, htree=True, clique_dim=CLIQUE_DIM)
        legs["pipeline_htree"] = lambda: plain.convert(*arrays)
        if HAS_MODE:
            typed = dsg.FramePipeline(DEV, htree=True, htree_relative_pos=True, clique_dim=CLIQUE_DIM)
            homog = dsg.FramePipeline(DEV, htree=True, htree_relative_pos=True, clique_dim=CLIQUE_DIM, homogeneous=True)

            def python_typed():
                rog = dsg.RoomObjectGraph(sg)
                g = dsg.to_hetero_data(rog, dsg.object_connectivity(rog, 1.5, 2.0, 0.2, DEV), None, DEV)
                tree = htree.generate_htree(g, clique_dim=CLIQUE_DIM, clique_pos=True)
                hdata.compute_relative_pos(tree)
                return tree

            legs["python_typed"] = python_typed
            legs["python_homogeneous"] = lambda: hdata.heterogeneous_htree_to_homogeneous(python_typed().to("cpu")).to(DEV)
            legs["pipeline_htree_relpos"] = lambda: typed.convert(*arrays)
            legs["pipeline_htree_relpos_homogeneous"] = lambda: homog.convert(*arrays)
            if args.convert_loop:
                for _ in range(args.convert_loop):
                    typed.convert(*arrays)
                    homog.convert(*arrays)
                torch.cuda.synchronize()
                continue
        for rnd in range(args.rounds):
            for leg, fn in legs.items():
                print(json.dumps({"tag": args.tag, "frame": name, "leg": leg, "round": rnd, "reps": args.reps, **timed(fn, args.reps)}), flush=True)


main()
