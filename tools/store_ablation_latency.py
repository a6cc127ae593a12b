#!/usr/bin/env python3
"""The edge-type and clique ablations on a resident dataset against the host route, on one MI355X.

The dataset is ``GraphStore.from_frames`` over ``--graphs`` (default 384) copies of the reference's test scene graph (the fixture: 62
kept objects, 5 rooms) with a 300-d semantic table, i.e. MP3D-like 306 / 6-wide features, as a typed baseline store and as a typed
H-tree store, and the homogeneous store derived from each.  Per derivation two legs are timed to completion (host call +
``torch.cuda.synchronize()``):

  device  the ``GraphStore`` method (``without_edge_types``, ``to_homogeneous(removed_edge_type=)``, ``zero_clique_features``): numpy
          planning, one upload, one ``hmp_store_derive`` launch; on a homogeneous store ``without_edge_types`` also runs the count
          launch and reads ``G`` int64 back
  host    the host transform of every graph (``data.remove_edge_types`` / ``data.heterogeneous_data_to_homogeneous(removed_edge_type=)``
          / ``data.zero_clique_features``), then ``GraphStore(list)``.  The host graphs exist already (their construction is not
          timed); each call works on fresh containers over the same tensors.

A figure is the median in microseconds of ``--reps`` (device) / ``--host-reps`` (host) calls after one warm-up call.  Prints one JSON
line per store kind; ``--out FILE`` appends them.  A measurement needs the GPU: without one the tool fails.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hydra-gnn_amd")]

RR = ("rooms", "rooms_to_rooms", "rooms")
RO = ("rooms", "rooms_to_objects", "objects")


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

    def homog(g, removed=None):
        if "object_virtual" in g.node_types:
            return data.heterogeneous_htree_to_homogeneous(g)
        d, types = data.heterogeneous_data_to_homogeneous(g, removed_edge_type=removed)
        d.room_mask = d.node_type == types.index("rooms")
        return d

    kinds = {"typed_baseline": dict(), "typed_htree": dict(htree=True, clique_dim=6)}
    for kind, kw in kinds.items():
        pipe = dsg.FramePipeline(dev, semantic_table=table, **kw)
        store, _ = GraphStore.from_frames(pipe, [arrays] * a.graphs, [y] * a.graphs)
        hstore = store.to_homogeneous()
        one = pipe.convert(*arrays)[0].to("cpu")
        for t in one.node_types:  # host graphs with the labels the store carries (all graphs are the same frame)
            if "y" in store.node_attrs[t]:
                one[t].y = store.node_attrs[t]["y"].data[:int(store.node_counts[t][0])].cpu()
        hosts = [one] * a.graphs
        fresh = lambda: [g.to("cpu") for g in hosts]  # new containers, the same tensors
        if kind == "typed_baseline":
            ro = store.edge_types.index(RO)
            legs = {
                "without_edge_types_rr_typed": (lambda: store.without_edge_types([RR]),
                                                lambda: GraphStore([data.remove_edge_types(g, [RR]) for g in fresh()], dev)),
                "to_homogeneous_removed_ro": (lambda: store.to_homogeneous(removed_edge_type=RO),
                                              lambda: GraphStore([homog(g, RO) for g in fresh()], dev)),
                "without_edge_types_ro_homogeneous": (lambda: hstore.without_edge_types([ro]),
                                                      lambda: GraphStore([data.remove_edge_types(homog(g), [ro]) for g in fresh()], dev)),
            }
        else:
            legs = {
                "zero_clique_features_typed": (lambda: store.zero_clique_features(),
                                               lambda: GraphStore([data.zero_clique_features(g) for g in fresh()], dev)),
                "zero_clique_features_homogeneous": (lambda: hstore.zero_clique_features(),
                                                     lambda: GraphStore([data.zero_clique_features(homog(g)) for g in fresh()], dev)),
                "without_edge_types_0_homogeneous": (lambda: hstore.without_edge_types([0]),
                                                     lambda: GraphStore([data.remove_edge_types(homog(g), [0]) for g in fresh()], dev)),
            }
        rec = {"tool": "store_ablation_latency", "kind": kind, "graphs": a.graphs, "reps": a.reps, "host_reps": a.host_reps,
               "edges": int(hstore.edge_ptr_host[hstore.edge_types[0]][-1]), "nodes": int(hstore.node_counts["node"].sum()), "legs": {}}
        for name, (device_fn, host_fn) in legs.items():
            d, h = timed(device_fn, a.reps), timed(host_fn, a.host_reps)
            rec["legs"][name] = {"device_us": d, "host_us": h, "ratio": round(h / d, 1)}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
