"""csrc/htree.cpp on scene graphs whose room layer has no edges (what ``remove_room_edges_in_dsg`` leaves: the ``noRE`` configurations
and ``FramePipeline(remove_room_edges=True)``) against H-trees built by the REFERENCE's junction-tree code
(tests/golden/htree_nore_reference_cases.npz, made by tests/golden/make_htree_nore_fixture.py): multi-room scenes, every room its own
component, no ``room-room`` clique.  The five tie-free cases must give the reference's labelled tree, the loopy one must satisfy the
construction rules (``test_htree_native.py`` holds the comparison and the rules).  Host code only: runs without a GPU."""
import os

import numpy as np
import pytest
import torch

from hydra_gnn_amd import htree
from test_htree_native import check_rules, signature

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "htree_nore_reference_cases.npz")
TIE_FREE = {"paths": [3, 4, 2], "stars": [5, 4], "singletons": [1, 1, 1], "rtrees": [6, 7, 5, 4], "isolated_objects": [3, 2]}
LOOPY = {"loopy": [8, 7, 6]}


def load(name):
    z = np.load(GOLDEN)
    n_obj, n_rooms = [int(v) for v in z[f"{name}_n"]]
    scene = (n_obj, n_rooms, torch.from_numpy(z[f"{name}_oo"]), torch.from_numpy(z[f"{name}_rr"]), torch.from_numpy(z[f"{name}_ro"]))
    ref = {"counts": z[f"{name}_counts"].tolist(), "object_orig": z[f"{name}_object_orig"], "room_orig": z[f"{name}_room_orig"],
           "edges": [z[f"{name}_e{k}"].reshape(2, -1) for k in range(10)], "init": [z[f"{name}_i{k}"].reshape(2, -1) for k in range(3)]}
    return scene, ref


def check_no_room_layer(scene, t, sizes):
    n_obj, n_rooms, oo, rr, ro = scene
    assert rr.shape == (2, 0) and n_rooms == len(sizes) > 1 and n_obj == sum(sizes)
    assert t["counts"][3] == 0  # no room-room clique ...
    for k in (4, 5, 6, 7, 9):  # ... and no edge that touches one
        assert np.asarray(t["edges"][k]).size == 0, k
    assert np.asarray(t["init"][2]).size == 0
    assert set(int(r) for r in t["room_orig"]) == set(range(n_rooms))


def test_the_fixture_holds_the_six_cases():
    assert np.load(GOLDEN)["names"].tolist() == list(TIE_FREE) + list(LOOPY)
    assert os.path.getsize(GOLDEN) < 64 * 1024


@pytest.mark.parametrize("name", list(TIE_FREE))
def test_tie_free_scenes_give_the_reference_htree(name):
    scene, ref = load(name)
    t = htree.htree_topology(*scene)
    check_rules(scene, t)
    check_rules(scene, ref)
    check_no_room_layer(scene, t, TIE_FREE[name])
    check_no_room_layer(scene, ref, TIE_FREE[name])
    assert t["counts"] == ref["counts"]
    assert signature(t) == signature(ref)


@pytest.mark.parametrize("name", list(LOOPY))
def test_the_loopy_scene_satisfies_the_construction_rules(name):
    scene, ref = load(name)
    t = htree.htree_topology(*scene)
    check_rules(scene, t)
    check_rules(scene, ref)
    check_no_room_layer(scene, t, LOOPY[name])
    check_no_room_layer(scene, ref, LOOPY[name])
    assert set(t["object_orig"].tolist()) == set(ref["object_orig"].tolist())
    print(f"{name}: native {t['counts']} reference {ref['counts']} identical labelled tree: {signature(t) == signature(ref)}")


def test_generate_htree_of_a_graph_without_room_edges():
    """the host oracle of the frames: ``data.remove_edge_types(g, [rooms_to_rooms])`` then ``generate_htree``"""
    from hydra_gnn_amd import data as hdata, workloads

    g = workloads.mp3d_like_graph(np.random.default_rng(3), mean_in_degree=2.0)
    assert g["rooms"].x.size(0) > 1 and g[htree.RR].edge_index.size(1) > 0
    full = htree.generate_htree(g)
    hdata.remove_edge_types(g, [htree.RR])
    t = htree.generate_htree(g)
    assert full["room-room"].x.size(0) > 0 and t["room-room"].x.size(0) == 0
    assert t["room", "r_to_rr", "room-room"].edge_index.shape == (2, 0) and t["room_virtual", "rv_to_rr", "room-room"].edge_index.shape == (2, 0)
    rv = t["room_virtual", "rv_to_or", "object-room"].edge_index
    assert torch.equal(t["object-room"].x[rv[1], :3], g["rooms"].x[rv[0], :3])  # one room per clique: its position, exactly
