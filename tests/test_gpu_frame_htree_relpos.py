"""Relative positions on H-tree edges on the device: ``FramePipeline(htree=True, htree_relative_pos=True)`` -- ``convert``,
``convert_batch`` and ``GraphStore.from_frames``, typed and homogeneous -- against the Python oracle
(``data.compute_relative_pos`` of ``htree.generate_htree(..., clique_pos=True)``), against the pipeline's own ``pos`` tensors (bit for
bit on all 15 edge types), and under the GAT_edge H-tree models that read the result."""
import numpy as np
import pytest
import torch

import _frame_batch_cases as bc
import _frame_cases as fc
import _frame_htree_relpos_cases as hc
from hydra_gnn_amd import _lib, data as hdata, dsg
from hydra_gnn_amd.models import HeterogeneousNeuralTreeNetwork, HomogeneousNeuralTreeNetwork
from hydra_gnn_amd.store import GraphStore
from test_gpu_frame_store import assert_same_store

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_PIPES, _ORACLE = {}, {}


def pipeline(homogeneous, which="main"):
    if (homogeneous, which) not in _PIPES:
        _PIPES[(homogeneous, which)] = dsg.FramePipeline(DEV, **hc.pipeline_kwargs(homogeneous))
    return _PIPES[(homogeneous, which)]


def oracle(name):
    """the oracle, computed once on the CPU: (typed tree, per-clique bounds)"""
    if str(name) not in _ORACLE:
        tree, members, rpos = hc.oracle_typed(hc.frame(name))
        _ORACLE[str(name)] = (tree, {t: hc.clique_bound(members[t], rpos) for t in hc.CLIQUE_TYPES})
    return _ORACLE[str(name)]


def assert_close_rows(got, want, bound, what):
    """``hc.assert_close_rows`` for a device tensor against the oracle moved to the device"""
    assert got.device == want.device and got.is_contiguous() and got.dtype == want.dtype and got.shape == want.shape, what
    exact = torch.from_numpy(bound == 0).to(got.device)
    assert torch.equal(got[exact], want[exact]), what
    if not bool(exact.all()):
        b = torch.from_numpy(bound).to(got.device)[~exact, None]
        assert bool(((got[~exact].double() - want[~exact].double()).abs() <= b).all()), what


def typed_copy(g):
    """a HeteroData from COPIES of a typed pipeline result's x, pos, label and edge lists, its edge_attr recomputed with the torch
    ops of ``data.compute_relative_pos`` (the pipeline's x went without the three columns already)"""
    out = hdata.HeteroData()
    for t in g.node_types:
        for attr, v in g[t].items():
            setattr(out[t], attr, v.clone())
    for e in g.edge_types:
        ei = g[e].edge_index.clone()
        out[e].edge_index = ei
        out[e].edge_attr = out[e[2]].pos[ei[1]] - out[e[0]].pos[ei[0]]
    return out


# ---- single frames ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hc.CASES, ids=str)
def test_convert_typed(name):
    tree, bounds = oracle(name)
    want = tree.to(DEV)
    got, info = pipeline(False).convert(*hc.frame(name))
    assert got.node_types == want.node_types and got.edge_types == want.edge_types
    for key in want.node_types + want.edge_types:
        assert sorted(got[key].keys()) == sorted(want[key].keys()), key
        for attr, w in want[key].items():
            g = getattr(got[key], attr)
            if attr == "edge_attr":
                assert_close_rows(g, w, hc.edge_bound(key, tree[key].edge_index.numpy(), bounds), (key, attr))
            elif attr == "pos" and key in bounds:
                assert_close_rows(g, w, bounds[key], (key, attr))
            else:
                assert g.dtype == w.dtype and g.shape == w.shape and g.is_contiguous() and torch.equal(g, w), (key, attr)
    for e in got.edge_types:  # against the pipeline's own pos tensors: bit for bit, all 15 edge types
        ei = got[e].edge_index
        assert got[e].edge_attr.shape == (ei.size(1), 3) and torch.equal(got[e].edge_attr, got[e[2]].pos[ei[1]] - got[e[0]].pos[ei[0]]), e
    for e in hc.POOL_KEYS:
        ea = got[e].edge_attr
        assert ea.numel() > 0 and not bool(ea.any()) and not bool(torch.signbit(ea).any())
    for t in hc.CLIQUE_TYPES:
        assert got[t].x.shape[1] == hc.CLIQUE_DIM - 3 and not bool(got[t].x.any())
    assert info["room_ids"].size == got["room_virtual"].x.size(0)


@pytest.mark.parametrize("name", hc.CASES, ids=str)
def test_convert_homogeneous(name):
    tree, members, rpos = hc.oracle_typed(hc.frame(name))  # heterogeneous_htree_to_homogeneous edits its argument: a fresh one
    bounds = {t: hc.clique_bound(members[t], rpos) for t in hc.CLIQUE_TYPES}
    eb = np.concatenate([hc.edge_bound(tuple(k), tree[tuple(k)].edge_index.numpy(), bounds) for k in hc.EDGE_KEYS[:10]])
    want = hdata.heterogeneous_htree_to_homogeneous(tree).to(DEV)
    got, _ = pipeline(True).convert(*hc.frame(name))
    typed, _ = pipeline(False).convert(*hc.frame(name))
    own = hdata.heterogeneous_htree_to_homogeneous(typed_copy(typed).to("cpu")).to(DEV)  # from the typed pipeline's output: bit for bit
    names = sorted(k for k, v in vars(want).items() if isinstance(v, torch.Tensor))
    assert names == sorted(k for k, v in vars(got).items() if isinstance(v, torch.Tensor)) and "edge_attr" in names
    for k in names:
        g, w = getattr(got, k), getattr(want, k)
        if k == "edge_attr":
            assert_close_rows(g, w, eb, k)
        else:
            assert g.dtype == w.dtype and g.shape == w.shape and g.is_contiguous() and torch.equal(g, w), k
        assert torch.equal(g, getattr(own, k)), k


def test_scene_entry_and_fresh_tensor_objects():
    sg = fc.scene_graph(hc.frame("fixture"))
    for homogeneous in (False, True):
        pipe = pipeline(homogeneous)
        a, info_a = pipe.convert_scene(sg)
        held = tensors_of(a)
        b, info_b = pipe.convert(*hc.frame("fixture"))
        assert all(np.array_equal(info_a[k], info_b[k]) for k in info_a)
        for k, t in tensors_of(b).items():
            assert t is not held[k] and torch.equal(t, held[k]), k


def tensors_of(d):
    if hasattr(d, "node_types"):
        return {(key, attr): t for key in d.node_types + d.edge_types for attr, t in d[key].items() if isinstance(t, torch.Tensor)}
    return {k: t for k, t in vars(d).items() if isinstance(t, torch.Tensor)}


# ---- batches ---------------------------------------------------------------------------------------------------------------------
def labels_of(frame_list):
    return [bc.class_labels(a, i) for i, a in enumerate(frame_list)]


# one, two and three item groups (and six): a homogeneous frame has 59 items, a typed one 46 + 6 (+ 4 with y) and 21 for the batch
@pytest.mark.parametrize("homogeneous,names,with_y,groups", [
    (True, ["fixture"], False, 1), (True, ["triangle", (7, 2)], False, 2), (True, ["special", (1, 1), "fixture"], False, 3),
    (False, ["triangle"], False, 2), (False, [(65, 1), "triangle"], True, 3), (False, bc.FRAME_NAMES + ["triangle"], True, 6)], ids=str)
def test_convert_batch_equals_collate_of_the_single_frames(homogeneous, names, with_y, groups):
    fr = [hc.frame(n) for n in names]
    ys = labels_of(fr) if with_y else None
    graphs, infos = bc.single_frame_clones(pipeline(homogeneous, "single"), fr, ys)
    want = bc.collate(graphs, homogeneous).to(DEV)
    pipe = pipeline(homogeneous)
    got, got_infos = pipe.convert_batch(fr, ys)
    n_items = len(graphs) * ((59 + (6 if with_y else 0)) if homogeneous else (46 + 6 + (4 if with_y else 0))) + (0 if homogeneous else 21)
    assert -(-n_items // 64) == groups
    bc.assert_same_batch(got, want)
    live = [i for i in got_infos if i is not None]
    assert [i is None for i in got_infos] == [i is None for i in infos] and [i["graph"] for i in live] == list(range(len(graphs)))
    if not homogeneous:
        assert sum("edge_attr" in got[e] for e in got.edge_types) == 15 and "pos" in got["object-room"] and "pos" in got["room-room"]


@pytest.mark.parametrize("homogeneous", [False, True], ids=["typed", "homogeneous"])
def test_store_from_frames_equals_the_store_over_the_single_frames(homogeneous):
    fr = [hc.frame(n) for n in bc.FRAME_NAMES + ["triangle"]]
    got, infos = GraphStore.from_frames(dsg.FramePipeline(DEV, **hc.pipeline_kwargs(homogeneous)), fr, labels_of(fr))
    graphs, _ = bc.single_frame_clones(pipeline(homogeneous, "single"), fr, labels_of(fr))
    want = GraphStore(graphs, DEV)
    assert_same_store(got, want)
    assert got.n_graphs == 6 and [None if i is None else i["graph"] for i in infos] == [0, 1, None, 2, 3, 4, 5]
    if homogeneous:
        assert len(got.edge_attr) == 1  # of edge_index: the ten tree edge types
    else:
        assert sorted(map(str, got.edge_attr)) == sorted(map(str, hc.EDGE_KEYS))  # the edge_attr of every edge type the frames carry
    ids = [5, 0, 3, 5]
    a, b = got.collate(ids), want.collate(ids)
    if not homogeneous:
        a.max_graph_nodes = b.max_graph_nodes = 0  # GraphStore.collate sets none
    bc.assert_same_batch(a, b)


GAT = dict(conv_block="GAT_edge", GAT_hidden_dims=[16, 16], GAT_heads=[2, 2, 2], GAT_concats=[True, True, False], dropout=0.25,
           disable_initialization=True)
DIMS = {t: 3 for t in dsg._HTREE_STORES}  # the frame's 6-d features after the three position columns are dropped


def model(homogeneous, two_headed=False):
    torch.manual_seed(0)
    if homogeneous:
        return HomogeneousNeuralTreeNetwork(3, output_dim=26, **GAT).to(DEV)
    if two_headed:
        return HeterogeneousNeuralTreeNetwork(dict(DIMS), output_dim_dict={"room": 26, "object": 26, "object-room": 1, "room-room": 1}, **GAT).to(DEV)
    return HeterogeneousNeuralTreeNetwork(dict(DIMS), output_dim=26, **GAT).to(DEV)


@pytest.mark.parametrize("homogeneous", [False, True], ids=["typed", "homogeneous"])
def test_gat_edge_models_read_the_pipeline_output(homogeneous):
    """logits and labels on the pipeline's result == on a graph assembled from copies of its x, pos and edge lists with edge_attr
    recomputed by torch"""
    net = model(homogeneous).eval()
    for name in ("fixture", "triangle"):
        got, info = pipeline(homogeneous).convert(*hc.frame(name))
        logits = net(got).clone()
        labels = net.predict(got).clone()
        typed, _ = pipeline(False, "single").convert(*hc.frame(name))
        ref = typed_copy(typed)
        if homogeneous:
            ref = hdata.heterogeneous_htree_to_homogeneous(ref.to("cpu")).to(DEV)
        assert torch.equal(net(ref), logits) and logits.shape == (info["room_ids"].size, 26) and bool(torch.isfinite(logits).all())
        assert torch.equal(net.predict(ref), labels)
    # the edge attributes are read: other values, other logits
    if homogeneous:
        ref.edge_attr = ref.edge_attr + 1.0
    else:
        for e in ref.edge_types:
            ref[e].edge_attr = ref[e].edge_attr + 1.0
    assert not torch.equal(net(ref), logits)


@pytest.mark.parametrize("kind", ["typed", "typed_two_headed", "homogeneous"])
def test_a_stream_batch_of_a_from_frames_store_and_a_training_step(kind):
    """the streamed batch of a GAT_edge H-tree net equals ``store.collate(ids)`` in everything it carries -- the ``edge_attr`` of the
    ten tree edge types included -- and one fused step on it ends with status 0 and a finite loss"""
    homogeneous = kind == "homogeneous"
    fr = [hc.frame(n) for n in ["fixture", "triangle", (7, 2), "special"]]
    store, _ = GraphStore.from_frames(dsg.FramePipeline(DEV, **hc.pipeline_kwargs(homogeneous)), fr, labels_of(fr))
    net = model(homogeneous, two_headed=kind == "typed_two_headed").train()
    ids = [2, 0, 3]
    if homogeneous:
        stream = store.stream(net, 3, "node", ignored_label=25)
    elif kind == "typed":  # the store holds 50 arrays, the collator's table 40: the stream carries what the net reads and the labels
        stream = store.stream(net, 3, "room_virtual")
    else:
        stream = store.stream(net, 3, masks=())
    h = stream.next(ids)
    want, seen = store.collate(ids), stream.data()
    carried = [(key, name) for _, key, name in stream._what]
    assert len(carried) <= _lib.COLLATE_MAX_ITEMS and sum(name == "edge_attr" for _, name in carried) == (1 if homogeneous else 10)
    if homogeneous:
        from hydra_gnn_amd.store import HOMO_NODE, homo_edge_type

        e0 = homo_edge_type("edge_index")
        assert torch.equal(seen[HOMO_NODE].x, want.x) and torch.equal(seen[HOMO_NODE].room_mask, want.room_mask)
        assert torch.equal(seen[HOMO_NODE].y, torch.where(want.room_mask, want.y, torch.full_like(want.y, 25)))
        assert torch.equal(seen[e0].edge_index, want.edge_index)
        assert seen[e0].edge_attr.shape == (want.edge_index.size(1), 3) and torch.equal(seen[e0].edge_attr, want.edge_attr)
        assert torch.equal(seen[homo_edge_type("pool_edge_index")].edge_index, want.pool_edge_index)
    else:
        for key, name in carried:
            assert torch.equal(getattr(seen[key], name), getattr(want[key], name)), (key, name)
        for e in hc.EDGE_KEYS[:10]:  # every message-passing edge type: its list and its attributes
            assert (tuple(e), "edge_index") in carried and (tuple(e), "edge_attr") in carried, e
        assert ("room_virtual", "y") in carried and all((t, "x") in carried for t in ("object", "room", "object-room", "room-room"))
    if kind == "typed_two_headed":
        step = net.semisupervised_step(lr=0.002, weight_decay=0.001, use_graph=False)
        step.run(h, mask=None)
    else:
        step = net.train_step(lr=0.002, weight_decay=0.001, ignored_label=25, seed=3, use_graph=False)
        step.run(h)
    assert np.isfinite(step.loss()) and net.native().read_state() == (1, 0)


def test_a_stream_of_every_array_still_carries_every_array():
    """a single-headed typed stream over a store that fits the collator's table carries all of it, as before"""
    fr = [hc.frame(n) for n in ["fixture", "triangle", (7, 2), "special"]]
    store, _ = GraphStore.from_frames(dsg.FramePipeline(DEV, htree=True, clique_dim=hc.CLIQUE_DIM), fr, labels_of(fr))
    torch.manual_seed(0)
    net = HeterogeneousNeuralTreeNetwork({t: 6 for t in dsg._HTREE_STORES}, output_dim=26, conv_block="GraphSAGE", hidden_dim=16, num_layers=3,
                                         disable_initialization=True, dropout=0.25).to(DEV)
    stream = store.stream(net, 2, "room_virtual")
    assert len(stream._what) == sum(len(a) for a in store.node_attrs.values()) + 15 == 33


# ---- what holds for every mode of the pipeline -----------------------------------------------------------------------------------
def test_arena_growth():
    pipe = dsg.FramePipeline(DEV, **hc.pipeline_kwargs(False))
    small, _ = pipe.convert(*hc.frame((7, 2)))
    held = {k: t.clone() for k, t in tensors_of(small).items()}
    arena, staging = pipe._arena.numel(), pipe._d_staging.numel()
    large, _ = pipe.convert(*hc.frame((300, 3)))  # fits neither the first arena (256 KiB) nor the first block (64 KiB)
    assert pipe._arena.numel() > arena and pipe._d_staging.numel() > staging
    ei = large["object", "o_to_or", "object-room"].edge_index
    assert torch.equal(large["object", "o_to_or", "object-room"].edge_attr, large["object-room"].pos[ei[1]] - large["object"].pos[ei[0]])
    again, _ = pipe.convert(*hc.frame((7, 2)))
    for k, t in tensors_of(again).items():
        assert torch.equal(t, held[k]), k


def test_another_stream_is_refused():
    pipe = dsg.FramePipeline(DEV, **hc.pipeline_kwargs(True))
    first, _ = pipe.convert(*hc.frame((7, 2)))
    held = first.edge_attr.clone()
    with torch.cuda.stream(torch.cuda.Stream(DEV)):
        with pytest.raises(_lib.HydraMPError, match="stream"):
            pipe.convert(*hc.frame((7, 2)))
    again, _ = pipe.convert(*hc.frame((7, 2)))  # back on the pipeline's stream
    assert torch.equal(again.edge_attr, held)
