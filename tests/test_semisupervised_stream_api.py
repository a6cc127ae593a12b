"""Device-free side of the two-headed stream: the per-graph generators of workloads.py, the naming of homogeneous edge lists in
the store, the public signatures, and the header's record of the relaxed row size."""
import inspect
import os

import pytest
import torch

from hydra_gnn_amd import evaluate, store, workloads
from hydra_gnn_amd.data import collate, collate_homogeneous
from hydra_gnn_amd.engine import LinearHeadTrainStep, TwoHeadTrainStep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASKS = ("train_mask", "val_mask", "test_mask")


def check_split(holder, n):
    tr, va, te = (getattr(holder, m) for m in MASKS)
    for m in (tr, va, te):
        assert m.dtype == torch.bool and m.shape == (n,)
    assert bool((tr.int() + va.int() + te.int() == 1).all())


@pytest.mark.parametrize("relative_pos", [False, True])
def test_hetero_generators_carry_their_masks_per_graph(relative_pos):
    gs = workloads.semisupervised_graphs(5, seed=2, relative_pos=relative_pos)
    hs = workloads.semisupervised_htree_graphs(5, seed=2, relative_pos=relative_pos)
    for g in gs:
        for t in ("rooms", "objects"):
            check_split(g[t], int(g[t].y.numel()))
        assert ("edge_attr" in g["objects", "objects_to_objects", "objects"]) == relative_pos
    for g in hs:
        for t, classes in (("room_virtual", 15), ("object_virtual", 35)):
            check_split(g[t], int(g[t].num_nodes))
            assert g[t].y.dtype == torch.int64 and int(g[t].y.max()) < classes
        assert ("edge_attr" in g["object", "o_to_or", "object-room"]) == relative_pos
        assert "edge_attr" not in g["room", "r_to_rv", "room_virtual"]
    again = workloads.semisupervised_graphs(5, seed=2, relative_pos=relative_pos)
    assert all(torch.equal(a["rooms"].train_mask, b["rooms"].train_mask) and torch.equal(a["objects"].x, b["objects"].x)
               for a, b in zip(gs, again))
    b = collate(gs)  # the host path of the task: masks are node attributes like any other
    assert b["objects"].val_mask.numel() == b["objects"].x.size(0)


def test_homogeneous_generators_carry_their_masks_per_graph():
    gs = workloads.stanford_semisupervised_graphs(6, seed=4, edge_attr=True)
    for g in gs:
        check_split(g, g.num_nodes)
        assert g.room_mask.dtype == torch.bool and int(g.room_mask.sum()) == 1
        assert g.edge_attr.shape == (g.edge_index.size(1), 3)
    hs = workloads.stanford_htree_semisupervised_graphs(4, seed=4)
    for g in hs:
        check_split(g, g.num_nodes)
        assert g.x.shape[1] == 6 and g.y.shape == (g.num_nodes,)
        assert int(g.y[g.room_mask].max()) < 15 and int(g.y.max()) < 35
        assert not bool((g.room_mask & g.object_mask).any())
        assert g.pool_edge_index.size(1) > 0 and g.init_edge_index.size(1) > 0
    b = collate_homogeneous(hs)
    assert b.train_mask.numel() == b.x.size(0) and int(b.pool_edge_index.max()) < b.x.size(0)


def test_existing_generators_are_untouched_by_the_new_ones():
    a = workloads.stanford_semisupervised_batch(5, seed=3)
    workloads.stanford_semisupervised_graphs(5, seed=3)
    b = workloads.stanford_semisupervised_batch(5, seed=3)
    assert torch.equal(a.x, b.x) and torch.equal(a.train_mask, b.train_mask)


def test_homogeneous_edge_lists_take_the_names_of_the_models_views():
    from hydra_gnn_amd.models.homogeneous_network import _EDGE, _NODE
    from hydra_gnn_amd.models.homogeneous_neural_tree_network import _INIT, _POOL

    assert store.HOMO_NODE == _NODE
    assert store.homo_edge_type("edge_index") == _EDGE
    assert store.homo_edge_type("pool_edge_index") == _POOL
    assert store.homo_edge_type("init_edge_index") == _INIT
    assert store.homo_edge_type("clique_index") == (_NODE, "clique", _NODE)


def test_signatures_read_like_the_room_task_ones():
    p = inspect.signature(store.GraphStore.stream).parameters
    assert list(p)[:4] == ["self", "net", "batch_size", "label_type"] and p["label_type"].default is None
    assert p["masks"].default == MASKS and p["targets"].default is True
    for cls in (TwoHeadTrainStep, LinearHeadTrainStep):
        q = inspect.signature(cls.run).parameters
        assert list(q) == ["self", "holder", "mask"] and q["mask"].default == "train_mask"
    r = inspect.signature(evaluate.semisupervised_accuracy).parameters
    assert list(r) == ["model", "batches", "mask_name", "type_separated"]
    assert r["mask_name"].default == "test_mask" and r["type_separated"].default is False
    with pytest.raises(ValueError):
        evaluate.semisupervised_accuracy(None, [], mask_name="room_mask")


def test_header_records_the_relaxed_row_size_and_the_item_capacity():
    with open(os.path.join(ROOT, "include", "hydra_mp.h")) as f:
        text = f.read()
    assert "multiple of 4); edges" not in text  # the old restriction on hmp_collate_item::row_bytes
    assert "40 items" in text and "264" in text
    with open(os.path.join(ROOT, "hydra-gnn_amd", "csrc", "collate.hip")) as f:
        src = f.read()
    assert "CB_MAX_ITEMS = 40" in src and "CB_INLINE_WORDS = 264" in src
    assert 264 >= 6 * 33 + 32  # the config-2 stream of 32 graphs keeps its tables in the argument block
