#!/usr/bin/env python3
"""Generates tests/golden/node_split_reference.npz -- masks written by the REFERENCE's own
``Stanford3DSG_dataset.generate_node_split`` (``src/hydra_gnn/Stanford3DSG_dataset.py:459-578``) on all four data types.

    python tests/golden/make_node_split_fixture.py PATH_TO_REFERENCE/src

The reference module imports ``torch_geometric`` (and, through ``preprocess_dsgs``, optionally ``spark_dsg``), which this project does
not depend on; ``generate_node_split`` itself only uses ``random``, ``torch`` and a handful of accessors of its data objects.  So the
module is imported with stand-in modules that provide the imported NAMES and nothing else, the dataset container is the reference's
own class, and the data objects are duck-typed: they answer ``num_graph_nodes()``, ``is_heterogeneous()``, ``get_torch_data()`` as
``Stanford3DSG_data`` / ``Stanford3DSG_htree_data`` do (``mp3d_dataset.py:331-339``, ``:407-417``), over this project's ``HeteroData`` / ``Data``.  The output is DATA only:
per case the node counts that define the graphs, the ratios and seed, and the three masks of every split node set, concatenated
over the graphs.  ``tests/test_store_derive_host.py`` replays the cases through the restated split.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "hydra-gnn_amd"))

from hydra_gnn_amd.data import Data, HeteroData  # noqa: E402

# (objects, rooms) of 6 graphs; one graph with a single room, one with a single object
COUNTS = [(5, 2), (3, 1), (1, 3), (7, 2), (4, 4), (2, 2)]
CASES = [("sum1", (0.7, 0.1, 0.2), 1), ("rest", (0.5, 0.2, None), 0), ("partial", (0.4, 0.2, 0.2), 3)]
DATA_TYPES = ["homogeneous", "heterogeneous", "homogeneous_htree", "heterogeneous_htree"]
HTREE_EXTRA = 3  # clique rows in front of / between the virtual rows of a homogeneous H-tree


def stand_in_modules():
    def module(name, **names):
        m = types.ModuleType(name)
        m.__dict__.update(names)
        sys.modules[name] = m
        return m

    def absent(*a, **k):
        raise RuntimeError("stand-in: not available")

    pyg = module("torch_geometric")
    pyg.data = module("torch_geometric.data", HeteroData=HeteroData, Data=Data)
    pyg.utils = module("torch_geometric.utils", is_undirected=absent, to_networkx=absent)


class Graph:
    """duck-typed Stanford3DSG_data / Stanford3DSG_htree_data"""

    def __init__(self, data_type, n_obj, n_room):
        self.data_type = data_type
        if data_type == "heterogeneous":
            d = HeteroData()
            d["objects"].x = torch.zeros(n_obj, 1)
            d["rooms"].x = torch.zeros(n_room, 1)
        elif data_type == "heterogeneous_htree":
            d = HeteroData()
            d["object_virtual"].x = torch.zeros(n_obj, 1)
            d["room_virtual"].x = torch.zeros(n_room, 1)
        elif data_type == "homogeneous":
            d = Data(x=torch.zeros(n_obj + n_room, 1))
        else:  # cliques, object_virtual rows, cliques, room_virtual rows, one clique
            n = HTREE_EXTRA + n_obj + HTREE_EXTRA + n_room + 1
            d = Data(x=torch.zeros(n, 1))
            d.object_mask = torch.zeros(n, dtype=torch.bool)
            d.room_mask = torch.zeros(n, dtype=torch.bool)
            d.object_mask[HTREE_EXTRA:HTREE_EXTRA + n_obj] = True
            d.room_mask[2 * HTREE_EXTRA + n_obj:2 * HTREE_EXTRA + n_obj + n_room] = True
        self._d, self._n = d, (n_obj, n_room)

    def is_heterogeneous(self):
        return self.data_type.startswith("heterogeneous")

    def get_torch_data(self):
        return self._d

    def num_graph_nodes(self):
        if self.data_type == "homogeneous_htree":  # :414-417
            return self._d.room_mask.sum().item() + self._d.object_mask.sum().item()
        return sum(self._n)


def main():
    stand_in_modules()
    sys.path.insert(0, sys.argv[1])
    from hydra_gnn.Stanford3DSG_dataset import Stanford3DSG_dataset  # the reference

    out = {"counts": np.array(COUNTS, dtype=np.int64), "htree_extra": np.array(HTREE_EXTRA)}
    for dt in DATA_TYPES:
        for name, ratios, seed in CASES:
            ds = Stanford3DSG_dataset()
            ds._data_list = [Graph(dt, *c) for c in COUNTS]
            ds.data_type = lambda dt=dt: dt  # the reference's data_type() inspects its own data classes
            ds.generate_node_split(*ratios, seed=seed)
            for m in ("train_mask", "val_mask", "test_mask"):
                if dt.startswith("heterogeneous"):
                    a, b = ("objects", "rooms") if dt == "heterogeneous" else ("object_virtual", "room_virtual")
                    for t in (a, b):
                        out[f"{dt}/{name}/{t}/{m}"] = torch.cat([getattr(g.get_torch_data()[t], m) for g in ds._data_list]).numpy()
                else:
                    out[f"{dt}/{name}/node/{m}"] = torch.cat([getattr(g.get_torch_data(), m) for g in ds._data_list]).numpy()
            out[f"{dt}/{name}/ratios"] = np.array([np.nan if r is None else r for r in ratios])
            out[f"{dt}/{name}/seed"] = np.array(seed)
    path = os.path.join(ROOT, "tests", "golden", "node_split_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays")


if __name__ == "__main__":
    main()
