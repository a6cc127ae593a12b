"""``dsg.FramePipeline.convert_batch`` on the device (csrc/frame.hip ``frame_expand_batch_kernel``: K frames, one upload, one launch)
against the pipeline's own single-frame path: ``data.collate`` / ``data.collate_homogeneous`` of the copies of ``convert(f)`` of
every frame, moved to the device.  Both sides come from the same kernel arithmetic (clique means included), so every tensor and
attribute is compared bit for bit.  Batches of one item group, across item 64 and of three and more groups; the pipeline's rules
(fresh tensor objects, arena growth, one stream, empty batches); and equal ``predict`` of three model classes."""
import numpy as np
import pytest
import torch

import _frame_batch_cases as bc
import _frame_cases as fc
from hydra_gnn_amd import _lib, dsg
from hydra_gnn_amd.models import HeterogeneousNetwork, HeterogeneousNeuralTreeNetwork, HomogeneousNetwork

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ["typed", "typed_htree", "homog", "homog_htree", "typed_relative_pos"]
_PIPES, _WANT = {}, {}


def pipeline(mode, which="batch"):
    """one pipeline per mode for the batched path and one for the single-frame path it is compared with"""
    if (mode, which) not in _PIPES:
        _PIPES[mode, which] = dsg.FramePipeline(DEV, **bc.pipeline_kwargs(mode))
    return _PIPES[mode, which]


def labels_of(frame_list):
    return [bc.labels(a, i) for i, a in enumerate(frame_list)]


def want(mode, names, with_y=True):
    """collate of the single-frame copies, on the device; computed once per case and left unchanged"""
    key = (mode, tuple(names), with_y)
    if key not in _WANT:
        fr = bc.frames(names)
        graphs, infos = bc.single_frame_clones(pipeline(mode, "single"), fr, labels_of(fr) if with_y else None)
        _WANT[key] = (bc.collate(graphs, bc.MODES[mode][0]).to(DEV), infos)
    return _WANT[key]


def n_items(mode, names, with_y=True):
    fr = bc.frames(names)
    return len(dsg.frame_batch_host_stage(fr, y=labels_of(fr) if with_y else None, **bc.host_kwargs(mode))["items"])


@pytest.mark.parametrize("mode", MODES)
def test_batch_equals_collate_of_the_single_frames(mode):
    fr = bc.frames()
    got, infos = pipeline(mode).convert_batch(fr, labels_of(fr))
    want_batch, want_infos = want(mode, bc.FRAME_NAMES)
    bc.assert_same_batch(got, want_batch)
    assert [None if i is None else i["graph"] for i in infos] == [0, 1, None, 2, 3, 4]
    for info, w in zip(infos, want_infos):
        assert (info is None) == (w is None)
        if w is not None:
            assert sorted(info) == sorted(list(w) + ["graph"]) and all(np.array_equal(info[k], w[k]) and info[k].dtype == w[k].dtype for k in w)
    got, _ = pipeline(mode).convert_batch(fr)  # without labels: no y anywhere
    bc.assert_same_batch(got, want(mode, bc.FRAME_NAMES, with_y=False)[0])


# one group of items; across item 64; three groups and more (the list repeated)
@pytest.mark.parametrize("mode,names,groups", [
    ("typed", [(7, 2), "fixture"], 1), ("homog", [(7, 2), "fixture", (1, 1), (65, 1)], 1), ("typed", bc.FRAME_NAMES, 2),
    ("homog", bc.FRAME_NAMES, 2), ("typed", bc.FRAME_NAMES * 2, 3), ("typed_htree", bc.FRAME_NAMES, 4), ("homog_htree", bc.FRAME_NAMES * 2, 9),
    ("homog_htree", [(1, 1)] * 6, 6)], ids=str)
def test_item_groups(mode, names, groups):
    assert -(-n_items(mode, names) // 64) == groups
    fr = bc.frames(names)
    got, _ = pipeline(mode).convert_batch(fr, labels_of(fr))
    bc.assert_same_batch(got, want(mode, names)[0])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["fixture", (1, 1)], ids=str)
def test_a_one_frame_batch_equals_convert(name, mode):
    arrays = bc.frame(name)
    got, infos = pipeline(mode).convert_batch([arrays])
    single, info = pipeline(mode, "single").convert(*arrays)
    assert got.num_graphs == 1 and infos[0]["graph"] == 0 and all(np.array_equal(infos[0][k], info[k]) for k in info)
    if bc.MODES[mode][0]:
        for k, v in vars(single).items():
            if isinstance(v, torch.Tensor):
                assert torch.equal(getattr(got, k), v), k
        return
    assert got.node_types == single.node_types and got.edge_types == single.edge_types
    for key in single.node_types + single.edge_types:
        for attr, w in single[key].items():
            assert torch.equal(getattr(got[key], attr), w), (key, attr)


def test_tensor_objects_are_fresh_on_every_call():
    fr = bc.frames([(7, 2), "fixture"])
    pipe = pipeline("typed")
    a, _ = pipe.convert_batch(fr)
    held = {(key, attr): t for key in a.node_types + a.edge_types for attr, t in a[key].items() if isinstance(t, torch.Tensor)}
    b, _ = pipe.convert_batch(fr)
    for (key, attr), t in held.items():
        assert getattr(b[key], attr) is not t and torch.equal(getattr(b[key], attr), t), (key, attr)
    pipe = pipeline("homog")
    a, _ = pipe.convert_batch(fr)
    b, _ = pipe.convert_batch(fr)
    for k, t in vars(a).items():
        if isinstance(t, torch.Tensor):
            assert getattr(b, k) is not t and torch.equal(getattr(b, k), t), k


def test_small_large_small_across_arena_growth():
    pipe = dsg.FramePipeline(DEV, **bc.pipeline_kwargs("typed_sem300"))
    small, large = [(7, 2), (1, 1)], bc.FRAME_NAMES * 4  # 306-d rows and 20 graphs: the large batch fits neither the first arena (256 KiB) nor the first block (64 KiB)
    got, _ = pipe.convert_batch(bc.frames(small))
    bc.assert_same_batch(got, want("typed_sem300", small, with_y=False)[0])
    arena, staging = pipe._arena.numel(), pipe._d_staging.numel()
    got, _ = pipe.convert_batch(bc.frames(large))
    assert pipe._arena.numel() > arena and pipe._d_staging.numel() > staging
    bc.assert_same_batch(got, want("typed_sem300", large, with_y=False)[0])
    got, _ = pipe.convert_batch(bc.frames(small))
    bc.assert_same_batch(got, want("typed_sem300", small, with_y=False)[0])


def test_another_stream_is_refused():
    pipe = dsg.FramePipeline(DEV)
    pipe.convert_batch(bc.frames([(7, 2)]))
    with torch.cuda.stream(torch.cuda.Stream(DEV)):
        with pytest.raises(_lib.HydraMPError, match="stream"):
            pipe.convert_batch(bc.frames([(7, 2)]))
    got, _ = pipe.convert_batch(bc.frames([(7, 2), (1, 1)]))  # back on the pipeline's stream
    bc.assert_same_batch(got, want("typed", [(7, 2), (1, 1)], with_y=False)[0])


@pytest.mark.parametrize("mode", ["typed", "homog_htree"])
def test_an_all_empty_batch_returns_none_without_touching_the_device(mode):
    pipe = dsg.FramePipeline(DEV, **bc.pipeline_kwargs(mode))
    fr = bc.frames(["no_room", "no_room"])
    batch, infos = pipe.convert_batch(fr, labels_of(fr))
    assert batch is None and infos == [None, None]
    assert pipe.convert_batch([]) == (None, [])
    assert pipe._arena is None and pipe._d_staging is None and pipe._stream is None


def test_more_items_than_a_launch_holds_is_refused():
    pipe = dsg.FramePipeline(DEV)
    pipe._batch_max_items = 64  # 4 typed frames need 4 * 14 + 6 = 62 items, 5 need 76
    assert pipe.convert_batch(bc.frames([(1, 1)] * 4))[0].num_graphs == 4
    with pytest.raises(_lib.HydraMPError, match="HMP_FRAME_BATCH_MAX_ITEMS"):
        pipe.convert_batch(bc.frames([(1, 1)] * 5))


@pytest.mark.parametrize("kind", ["sage", "htree", "homog"])
def test_models_predict_the_same_on_the_batch(kind):
    torch.manual_seed(0)
    if kind == "sage":
        mode, net = "typed", HeterogeneousNetwork(input_dim_dict={"objects": 6, "rooms": 6}, output_dim=26, conv_block="GraphSAGE", hidden_dim=64,
                                                  num_layers=3, dropout=0.25)
    elif kind == "htree":
        dims = {"object": 6, "room": 6, "object-room": 6, "room-room": 6, "object_virtual": 6, "room_virtual": 6}
        mode, net = "typed_htree", HeterogeneousNeuralTreeNetwork(dims, output_dim=26, conv_block="GraphSAGE", hidden_dim=32, num_layers=3,
                                                                  disable_initialization=True, dropout=0.25)
    else:
        mode, net = "homog", HomogeneousNetwork(6, output_dim=26, conv_block="GraphSAGE", hidden_dim=64, num_layers=3, dropout=0.25)
    net = net.to(DEV).eval()
    want_batch, infos = want(mode, bc.FRAME_NAMES, with_y=False)
    expected = net.predict(want_batch).clone()
    got_batch, _ = pipeline(mode).convert_batch(bc.frames())
    got = net.predict(got_batch).clone()
    assert expected.numel() == sum(i["room_ids"].size for i in infos if i is not None) and torch.equal(got, expected)


def test_expand_batch_refuses_bad_arguments():
    """the refusals of hmp_frame_expand with the larger item bound; every one comes before the launch"""
    lib = _lib.require_device()
    staging, arena = (torch.zeros(4096, dtype=torch.uint8, device=DEV) for _ in range(2))
    table = torch.zeros(64, dtype=torch.float32, device=DEV)
    s, a, t, st = staging.data_ptr(), arena.data_ptr(), table.data_ptr(), _lib.stream_ptr()
    for args in [(None, a, None, 0, 1, 1), (s, None, None, 0, 1, 1), (s + 8, a, None, 0, 1, 1), (s, a + 4, None, 0, 1, 1),
                 (s, a, None, 0, 0, 1), (s, a, None, 0, _lib.FRAME_BATCH_MAX_ITEMS + 1, 1), (s, a, None, 0, 1, 0), (s, a, None, -1, 1, 1),
                 (s, a, None, 8, 1, 1), (s, a, t + 4, 8, 1, 1)]:
        assert lib.hmp_frame_expand_batch(*args, st) == 1, args  # HMP_E_ARG
        assert b"hmp_frame_expand_batch" in lib.hmp_last_error()
    torch.cuda.synchronize()
    assert not arena.any()  # nothing was launched
