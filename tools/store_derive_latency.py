#!/usr/bin/env python3
"""Derived stores and the node split on a resident dataset against the host path, on one MI355X.

The dataset is ``GraphStore.from_frames`` over ``--graphs`` (default 384) copies of the reference's test scene graph (the fixture: 62
kept objects, 5 rooms) with a 300-d semantic table, i.e. MP3D-like 306 / 6-wide features, as a typed baseline store and as a typed
H-tree store.  Per transform two legs are timed to completion (host call + ``torch.cuda.synchronize()``):

  device  the ``GraphStore`` method: numpy planning over the store's offset vectors, one upload, one ``hmp_store_derive`` launch
  host    what the package offered before: the ``data.*`` function on every host graph, then ``GraphStore(list)`` (``torch.cat`` per
          attribute and the upload).  The host graphs exist already (their construction is not timed); each call works on fresh
          containers over the same tensors.

``generate_node_split`` has no host counterpart in the package; its figure stands alone (first call, which allocates the mask rows
and, for a homogeneous H-tree, reads the member counts once, and the median of the later calls).  A figure is the median in
microseconds of ``--reps`` (device) / ``--host-reps`` (host) calls after one warm-up call.  Prints one JSON line per store kind;
``--out FILE`` appends them.  A measurement needs the GPU: without one the tool fails.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hydra-gnn_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=384)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch

    from hydra_gnn_amd import _lib, data, dsg
    from hydra_gnn_amd.store import GraphStore

    _lib.require_device()
    dev = "cuda:0"
    arrays = dsg.scene_arrays(dsg.load_dsg_json(os.path.join(ROOT, "tests", "golden", "dsg_x8F5xyUWy9e.json")))
    y = (np.arange(arrays[0].size, dtype=np.int64) * 7) % 26
    table = torch.from_numpy(np.random.default_rng(0).normal(0.0, 0.15, size=(int(arrays[5].max()) + 1, 300)).astype(np.float32))

    def timed(fn, reps):
        out = []
        for it in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it:
                out.append((time.perf_counter() - t0) * 1e6)
        return round(float(np.median(out)), 1)

    def relpos(g):
        data.compute_relative_pos(g)
        return g

    def homog(g):
        if "object_virtual" in g.node_types:
            return data.heterogeneous_htree_to_homogeneous(g)
        d, types = data.heterogeneous_data_to_homogeneous(g)
        d.room_mask = d.node_type == types.index("rooms")
        return d

    def drop(g, dim):
        for t in g.x_dict:
            if g[t].num_node_features >= dim:
                g[t].x = g[t].x[:, :-dim]
        return g

    kinds = {"typed_baseline": dict(), "typed_htree": dict(htree=True, clique_dim=6)}
    for kind, kw in kinds.items():
        pipe = dsg.FramePipeline(dev, semantic_table=table, **kw)
        store, _ = GraphStore.from_frames(pipe, [arrays] * a.graphs, [y] * a.graphs)
        one = pipe.convert(*arrays)[0].to("cpu")
        # host graphs with the labels the store carries: read back from the store, graph 0 (all graphs are the same frame)
        for t in one.node_types:
            if "y" in store.node_attrs[t]:
                one[t].y = store.node_attrs[t]["y"].data[:int(store.node_counts[t][0])].cpu()
        hosts = [one] * a.graphs
        fresh = lambda: [g.to("cpu") for g in hosts]  # new containers, the same tensors
        legs = {"to_homogeneous": (lambda: store.to_homogeneous(), lambda: GraphStore([homog(g) for g in fresh()], dev)),
                "remove_last_features_300": (lambda: store.remove_last_features(300), lambda: GraphStore([drop(g, 300) for g in fresh()], dev))}
        if kind == "typed_baseline":  # the typed H-tree frames carry no clique positions
            legs["with_relative_pos"] = (lambda: store.with_relative_pos(), lambda: GraphStore([relpos(g) for g in fresh()], dev))
            legs["relative_pos_then_homogeneous"] = (lambda: store.with_relative_pos().to_homogeneous(),
                                                     lambda: GraphStore([homog(relpos(g)) for g in fresh()], dev))
        rec = {"tool": "store_derive_latency", "kind": kind, "graphs": a.graphs, "reps": a.reps, "host_reps": a.host_reps, "legs": {}}
        for name, (device_fn, host_fn) in legs.items():
            d, h = timed(device_fn, a.reps), timed(host_fn, a.host_reps)
            rec["legs"][name] = {"device_us": d, "host_us": h, "ratio": round(h / d, 1)}
        for name, s in (("typed", store), ("homogeneous", store.to_homogeneous())):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.generate_node_split(0.7, 0.1, 0.2, seed=0)
            torch.cuda.synchronize()
            first = round((time.perf_counter() - t0) * 1e6, 1)
            seeds = iter(range(1, a.reps + 3))
            rec["legs"][f"generate_node_split_{name}"] = {"first_call_us": first,
                                                          "device_us": timed(lambda: s.generate_node_split(0.7, 0.1, 0.2, seed=next(seeds)), a.reps)}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
