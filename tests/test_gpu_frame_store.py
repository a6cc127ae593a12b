"""``store.GraphStore.from_frames`` on the device: a store built from scene-graph arrays through the frame pipeline's batch path in
store form (csrc/frame.cpp ``HMP_FB_STORE``, one launch per chunk) against ``GraphStore`` over the copies of the pipeline's own
single-frame results.  Every packed array and offset vector is compared bit for bit; ``collate``, a ``stream`` batch with a training
step, and a frame list forced over several chunks behave as on the other store."""
import numpy as np
import pytest
import torch

import _frame_batch_cases as bc
from hydra_gnn_amd import _lib, dsg
from hydra_gnn_amd.models import HeterogeneousNetwork
from hydra_gnn_amd.store import GraphStore, _Packed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ["typed", "typed_htree", "homog", "homog_htree", "typed_relative_pos"]
_STORES = {}


def labels_of(frame_list):
    return [bc.class_labels(a, i) for i, a in enumerate(frame_list)]


def stores(mode):
    """(store from frames, infos, store over the single-frame copies), built once per mode"""
    if mode not in _STORES:
        fr = bc.frames()
        got, infos = GraphStore.from_frames(dsg.FramePipeline(DEV, **bc.pipeline_kwargs(mode)), fr, labels_of(fr))
        graphs, _ = bc.single_frame_clones(dsg.FramePipeline(DEV, **bc.pipeline_kwargs(mode)), fr, labels_of(fr))
        _STORES[mode] = (got, infos, GraphStore(graphs, DEV))
    return _STORES[mode]


def assert_same_value(g, w, what):
    if isinstance(w, _Packed):
        assert isinstance(g, _Packed)
        return assert_same_value(vars(g), vars(w), what)
    if isinstance(w, dict):
        assert list(g) == list(w), (what, list(g), list(w))  # same keys in the same order: collate walks them
        for k in w:
            assert_same_value(g[k], w[k], (what, k))
    elif isinstance(w, torch.Tensor):
        assert g.dtype == w.dtype and g.shape == w.shape and g.device == w.device and g.is_contiguous() and torch.equal(g, w), what
    elif isinstance(w, np.ndarray):
        assert g.dtype == w.dtype and np.array_equal(g, w), what
    else:
        assert g == w, what


def assert_same_store(got, want):
    skip = ("lib", "_stage", "_stage_dev", "_copied")
    assert sorted(k for k in vars(got) if k not in skip) == sorted(k for k in vars(want) if k not in skip)
    for k, w in vars(want).items():
        if k not in skip:
            assert_same_value(getattr(got, k), w, k)


@pytest.mark.parametrize("mode", MODES)
def test_store_equals_the_store_over_the_single_frames(mode):
    got, infos, want = stores(mode)
    assert_same_store(got, want)
    assert got.n_graphs == 5 and [None if i is None else i["graph"] for i in infos] == [0, 1, None, 2, 3, 4]
    ids = [3, 0, 3, 1]
    a, b = got.collate(ids), want.collate(ids)
    if bc.MODES[mode][0]:
        bc.assert_same_batch(a, b)
    else:
        a.max_graph_nodes = b.max_graph_nodes = 0  # GraphStore.collate sets none
        bc.assert_same_batch(a, b)


def test_the_store_owns_copies():
    pipe = dsg.FramePipeline(DEV)
    fr = bc.frames()
    got, _ = GraphStore.from_frames(pipe, fr, labels_of(fr))
    held = got.node_attrs["objects"]["x"].data.clone()
    pipe.convert_batch(bc.frames(["fixture", "fixture"]))  # rewrites the pipeline's arena
    assert torch.equal(got.node_attrs["objects"]["x"].data, held)
    lo, hi = pipe._arena.data_ptr(), pipe._arena.data_ptr() + pipe._arena.numel()
    assert not lo <= got.node_attrs["objects"]["x"].data.data_ptr() < hi


@pytest.mark.parametrize("mode", ["typed", "homog_htree"])
def test_a_frame_list_over_several_chunks_equals_one_chunk(mode):
    fr = bc.frames()
    pipe = dsg.FramePipeline(DEV, **bc.pipeline_kwargs(mode))
    pipe._batch_max_items = {"typed": 2 * 14 + 6, "homog_htree": 2 * 55 + 4}[mode]  # two frames per launch: chunks of 2, 2 and 1
    got, infos = GraphStore.from_frames(pipe, fr, labels_of(fr))
    assert_same_store(got, stores(mode)[0])
    assert [None if i is None else i["graph"] for i in infos] == [0, 1, None, 2, 3, 4]


def test_a_stream_batch_and_a_training_step():
    got, _, want = stores("typed")
    kw = dict(input_dim_dict={"objects": 6, "rooms": 6}, output_dim=26, conv_block="GraphSAGE", hidden_dim=64, num_layers=3, dropout=0.25)
    losses = []
    for store in (got, want):
        torch.manual_seed(0)
        net = HeterogeneousNetwork(**kw).to(DEV)
        net.train()
        step = net.train_step(lr=0.002, weight_decay=0.001, ignored_label=25, seed=3, use_graph=False)
        stream = store.stream(net, 2, "rooms")
        step.run(stream.next([4, 1]))
        losses.append(step.loss())
    assert np.isfinite(losses[0]) and losses[0] == losses[1]


def test_no_frame_with_items_is_refused():
    with pytest.raises(_lib.HydraMPError, match="no frame"):
        GraphStore.from_frames(dsg.FramePipeline(DEV), bc.frames(["no_room"]))
