"""The reference's ``Stanford3DSG_dataset.generate_node_split`` (``src/hydra_gnn/Stanford3DSG_dataset.py:459-578``) restated over this
project's host graphs (``data.HeteroData`` / ``data.Data``): the oracle of the store's node split.  Parity with the reference's own
code is pinned by ``tests/golden/node_split_reference.npz`` (``tests/test_store_derive_host.py``)."""
import random

import torch


def assignment_list(total, train_node_ratio, val_node_ratio, test_node_ratio, seed=0):
    """:462-492"""
    random.seed(seed)
    assert train_node_ratio > 0
    assert val_node_ratio >= 0
    if test_node_ratio is None:
        test_node_ratio = 1 - train_node_ratio - val_node_ratio
    assert test_node_ratio >= 0
    assert train_node_ratio + val_node_ratio + test_node_ratio <= 1
    num_train_nodes = round(total * train_node_ratio)
    num_val_nodes = round(total * val_node_ratio)
    if train_node_ratio + val_node_ratio + test_node_ratio == 1:
        num_test_nodes = total - num_train_nodes - num_val_nodes
        lst = [1] * num_train_nodes + [2] * num_val_nodes + [3] * num_test_nodes
    else:
        num_test_nodes = round(total * test_node_ratio)
        num_unassigned_nodes = total - num_train_nodes - num_val_nodes - num_test_nodes
        lst = [1] * num_train_nodes + [2] * num_val_nodes + [3] * num_test_nodes + [0] * num_unassigned_nodes
    random.shuffle(lst)
    return lst


def num_graph_nodes(g, data_type):
    """mp3d_dataset.py:331-339, Stanford3DSG_dataset.py:407-417"""
    if data_type == "heterogeneous":
        return g["objects"].num_nodes + g["rooms"].num_nodes
    if data_type == "heterogeneous_htree":
        return g["room_virtual"].num_nodes + g["object_virtual"].num_nodes
    if data_type == "homogeneous":
        return g.num_nodes
    return g.room_mask.sum().item() + g.object_mask.sum().item()


def generate_node_split(graphs, data_type, train_node_ratio, val_node_ratio, test_node_ratio, seed=0):
    """:459-578, in place on ``graphs``"""
    lst = assignment_list(sum(num_graph_nodes(g, data_type) for g in graphs), train_node_ratio, val_node_ratio, test_node_ratio, seed)
    names = (("train_mask", 1), ("val_mask", 2), ("test_mask", 3))
    for g in graphs:
        n = num_graph_nodes(g, data_type)
        node_split = torch.tensor(lst[:n], dtype=torch.int)
        lst = lst[n:]
        if data_type == "homogeneous":
            for name, v in names:
                setattr(g, name, node_split == v)
        elif data_type in ("heterogeneous", "heterogeneous_htree"):
            a, b = ("objects", "rooms") if data_type == "heterogeneous" else ("object_virtual", "room_virtual")
            num_objects = g[a].num_nodes
            for name, v in names:
                setattr(g[a], name, node_split[:num_objects] == v)
                setattr(g[b], name, node_split[num_objects:] == v)
        elif data_type == "homogeneous_htree":
            num_objects = g.object_mask.sum().item()
            for name, v in names:
                m = torch.zeros(g.num_nodes, dtype=torch.bool)
                m[g.object_mask] = (node_split == v)[:num_objects]
                m[g.room_mask] = (node_split == v)[num_objects:]
                setattr(g, name, m)
        else:
            raise NotImplementedError(data_type)
    assert len(lst) == 0
