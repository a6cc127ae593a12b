#!/usr/bin/env python3
"""Generates tests/golden/htree_nore_reference_cases.npz: H-trees built by the REFERENCE's own junction-tree-hierarchy code for
multi-room scene graphs whose room layer has NO edges -- what ``Hydra_mp3d_data.remove_room_edges_in_dsg`` leaves of a scene graph
before the H-tree is built (the ``noRE`` configurations).  Every room is its own component, so the tree holds no ``room-room`` clique.
tests/test_htree_nore.py compares csrc/htree.cpp against them.  The layout is that of htree_reference_cases.npz.

Run in the BUILD container only:  python tests/golden/make_htree_nore_fixture.py
"""
import os
import sys

import networkx as nx
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_htree_fixture as ref  # noqa: E402  (imports the reference's generate_junction_tree_hierarchies)
from make_htree_native_fixture import empty, path, rtree, scene, sparse, star  # noqa: E402

# name -> (objects per room, object graph of a room, seed); the room graph is always `empty`
CASES = {
    "paths": ([3, 4, 2], path, 0), "stars": ([5, 4], star, 1), "singletons": ([1, 1, 1], empty, 4), "rtrees": ([6, 7, 5, 4], rtree, 3),
    "isolated_objects": ([3, 2], empty, 6), "loopy": ([8, 7, 6], sparse, 8),
}


def main():
    out = {"names": np.array(list(CASES))}
    for name, (sizes, og, seed) in CASES.items():
        n_obj, n_rooms, oo, rr, ro = scene(sizes, og, empty, seed)
        assert rr == [] and n_rooms > 1
        G = nx.Graph()
        for i in range(n_obj):
            G.add_node(i, node_type="object", orig=i, x=[0.0], pos=[0.0] * 3, label=0)
        for r in range(n_rooms):
            G.add_node(n_obj + r, node_type="room", orig=r, x=[0.0], pos=[0.0] * 3, label=0)
        G.add_edges_from(oo)
        G.add_edges_from((n_obj + a, b) for a, b in ro)
        ht = ref.build_htree(G)
        per_type, leaf_orig, edges, init = ref.typed_arrays(G, ht)
        out[f"{name}_n"] = np.array([n_obj, n_rooms], dtype=np.int32)
        out[f"{name}_oo"] = np.array(oo, dtype=np.int64).reshape(-1, 2).T
        out[f"{name}_rr"] = np.array(rr, dtype=np.int64).reshape(-1, 2).T
        out[f"{name}_ro"] = np.array(ro, dtype=np.int64).reshape(-1, 2).T
        out[f"{name}_counts"] = np.array([len(per_type[t]) for t in ref.NODE_TYPES], dtype=np.int32)
        out[f"{name}_object_orig"] = leaf_orig["object"]
        out[f"{name}_room_orig"] = leaf_orig["room"]
        for k, et in enumerate(ref.EDGE_TYPES):
            out[f"{name}_e{k}"] = np.array(edges[et], dtype=np.int32).reshape(-1, 2).T
        for k, key in enumerate(("ov_to_or", "rv_to_or", "rv_to_rr")):
            out[f"{name}_i{k}"] = np.array(init[key], dtype=np.int32).reshape(-1, 2).T
        assert out[f"{name}_counts"][3] == 0, name  # no room-room clique
        print(name, "scene", n_obj, n_rooms, "-> htree", out[f"{name}_counts"].tolist())
    path_out = os.path.join(HERE, "htree_nore_reference_cases.npz")
    np.savez_compressed(path_out, **out)
    print("wrote", path_out, os.path.getsize(path_out), "bytes")


if __name__ == "__main__":
    main()
