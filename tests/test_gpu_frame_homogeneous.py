"""``dsg.FramePipeline(homogeneous=True)`` on the device (csrc/frame.hip: still one upload and one launch) against the committed
host conversion -- ``data.heterogeneous_data_to_homogeneous`` (+ ``room_mask``) / ``data.heterogeneous_htree_to_homogeneous`` --
applied to what the SAME pipeline returns with ``homogeneous=False``, moved to the CPU.  Both sides come from the same kernel
arithmetic (clique means included), so every tensor is compared bit for bit; the homogeneous models then give the same ``predict``
and ``forward`` on both, no plan is carried from one frame to the next, and a foreign stream is still refused."""
import numpy as np
import pytest
import torch

import _frame_cases as fc
from hydra_gnn_amd import _lib, dsg
from hydra_gnn_amd.data import Data, heterogeneous_data_to_homogeneous, heterogeneous_htree_to_homogeneous
from hydra_gnn_amd.models import HomogeneousNetwork, HomogeneousNeuralTreeNetwork

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FRAMES = ["fixture", "special", (1, 1), (7, 2)]
# name -> (htree, relative_pos, sem, clique_dim); clique_dim 16 with 6-wide leaves: the clique rows are the widest type
MODES = {"baseline": (False, False, False, None), "relative_pos": (False, True, False, None), "sem300": (False, False, True, None),
         "relative_pos_sem300": (False, True, True, None), "htree_c6": (True, False, False, 6), "htree_cNone": (True, False, False, None),
         "htree_c16": (True, False, False, 16), "htree_sem300_c6": (True, False, True, 6), "htree_sem300_cNone": (True, False, True, None)}
_PIPES = {}


def pipeline(mode, homogeneous):
    key = (mode, homogeneous)
    if key not in _PIPES:
        ht, rel, sem, cd = MODES[mode]
        _PIPES[key] = dsg.FramePipeline(DEV, semantic_table=fc.semantic_table() if sem else None, htree=ht, relative_pos=rel, clique_dim=cd,
                                        homogeneous=homogeneous)
    return _PIPES[key]


def host_conversion(frame_cpu, htree_mode) -> Data:
    """the committed host code on a typed frame that lives on the CPU"""
    if htree_mode:
        return heterogeneous_htree_to_homogeneous(frame_cpu)
    d, types = heterogeneous_data_to_homogeneous(frame_cpu)
    d.room_mask = d.node_type == types.index("rooms")  # Hydra_mp3d_data.to_homogeneous
    return d


def oracle(arrays, mode):
    """(Data on the CPU, info): typed pipeline -> CPU -> host conversion"""
    frame, info = pipeline(mode, False).convert(*arrays)
    return host_conversion(frame.to("cpu"), MODES[mode][0]), info


def attributes(d: Data):
    return {k: v for k, v in vars(d).items() if k != "_plan_cache"}


def assert_same_data(got: Data, want: Data):
    assert type(got) is Data
    g, w = attributes(got), attributes(want)
    assert sorted(g) == sorted(w)
    for k, t in w.items():
        assert g[k].dtype == t.dtype and g[k].shape == t.shape and g[k].is_contiguous() and g[k].device.type == "cuda", (k, g[k].dtype, g[k].shape)
        assert torch.equal(g[k].cpu(), t), k


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", FRAMES, ids=str)
def test_pipeline_against_pipeline(name, mode):
    arrays = fc.frame(name)
    want, want_info = oracle(arrays, mode)
    got, info = pipeline(mode, True).convert(*arrays)
    assert_same_data(got, want)
    assert sorted(info) == sorted(want_info) and all(np.array_equal(info[k], want_info[k]) and info[k].dtype == want_info[k].dtype for k in info)
    assert got.room_mask.dtype == torch.bool and int(got.room_mask.sum()) == info["room_ids"].size  # room_ids: the room_mask rows, in order
    ht, rel, sem, cd = MODES[mode]
    width = max((0 if rel else 3) + 3 + (300 if sem else 0), cd or 0)
    assert got.x.shape[1] == width and hasattr(got, "edge_attr") == rel and hasattr(got, "object_mask") == ht


def test_scene_entry_and_fixture_shapes():
    got, info = pipeline("htree_sem300_c6", True).convert_scene(dsg.load_dsg_json(fc.JSON))
    assert tuple(got.x.shape) == (268, 306) and tuple(got.edge_index.shape) == (2, 394)
    assert tuple(got.init_edge_index.shape) == (2, 195) and tuple(got.pool_edge_index.shape) == (2, 166)
    assert int(got.room_mask.sum()) == 5 and int(got.object_mask.sum()) == 62 and info["room_ids"].size == 5
    got, _ = pipeline("sem300", True).convert_scene(dsg.load_dsg_json(fc.JSON))
    assert tuple(got.x.shape) == (67, 306) and tuple(got.edge_index.shape) == (2, 482)
    assert torch.bincount(got.edge_type).tolist() == [356, 2, 62, 62]


# ---- the models read it ----------------------------------------------------------------------------------------------------------
def model(kind):
    torch.manual_seed(0)
    if kind == "sage306":
        return "sem300", HomogeneousNetwork(306, output_dim=26, conv_block="GraphSAGE", hidden_dim=64, num_layers=3, dropout=0.25)
    if kind == "gat_edge303":
        return "relative_pos_sem300", HomogeneousNetwork(303, output_dim=26, conv_block="GAT_edge", GAT_hidden_dims=[16, 16], GAT_heads=[2, 2, 2],
                                                         GAT_concats=[True, True, False], dropout=0.25)
    if kind == "htree_pre_mp":
        return "htree_c6", HomogeneousNeuralTreeNetwork(6, output_dim=26, conv_block="GraphSAGE", hidden_dim=16, num_layers=3, dropout=0.25)
    if kind == "htree_no_pre_mp":
        return "htree_sem300_c6", HomogeneousNeuralTreeNetwork(306, output_dim=26, conv_block="GraphSAGE", hidden_dim=32, num_layers=3,
                                                               disable_initialization=True, dropout=0.25)
    assert kind == "gcn_ops"
    return "baseline", HomogeneousNetwork(6, output_dim=26, conv_block="GCN", hidden_dim=32, num_layers=3, dropout=0.25)


@pytest.mark.parametrize("kind", ["sage306", "gat_edge303", "htree_pre_mp", "htree_no_pre_mp", "gcn_ops"])
def test_models_read_the_pipeline_output(kind):
    mode, net = model(kind)
    net = net.to(DEV).eval()
    for name in ("fixture", (7, 2)):
        arrays = fc.frame(name)
        want_data, _ = oracle(arrays, mode)
        want_data = want_data.to(DEV)
        got_data, info = pipeline(mode, True).convert(*arrays)
        assert got_data.x.shape[1] == net.input_dim
        with torch.no_grad():
            want, got = net(want_data).clone(), net(got_data).clone()
        assert want.shape == (info["room_ids"].size, 26) and torch.equal(got, want)
        if kind != "gcn_ops":  # the op path: forward() only
            want = net.predict(want_data).clone()
            got = net.predict(got_data).clone()
            assert want.numel() == info["room_ids"].size and want.dtype == torch.int64 and torch.equal(got, want)


def shifted_rooms_frame(shift):
    """6 rooms in a chain, one place each, 12 objects too far apart for any object edge: place k hangs off room (k + shift) % 6,
    so two shifts give the same node and edge COUNTS and different room-object edges"""
    sym = lambda c, i: (ord(c) << 56) + i
    rng = np.random.Generator(np.random.PCG64(4))
    ids, layer, pos, edges = [], [], [], []
    for k in range(6):
        ids += [sym("R", k), sym("p", k)]
        layer += [4, 3]
        pos += [[10.0 * k, 0, 0], [10.0 * k, 1, 0]]
        edges += [(sym("p", k), sym("R", (k + shift) % 6))] + ([(sym("R", k - 1), sym("R", k))] if k else [])
    for o in range(12):
        ids.append(sym("O", o)), layer.append(2), pos.append([10.0 * (o % 6) + rng.normal(), 5.0 * (o // 6) + 3, rng.normal()])
        edges.append((sym("O", o), sym("p", o % 6)))
    pos = np.array(pos, dtype=np.float64)
    return (np.array(ids, dtype=np.uint64), np.array(layer, dtype=np.int32), pos, pos - 0.2, pos + 0.2, np.arange(len(ids), dtype=np.int64) % 20,
            np.array(edges, dtype=np.uint64).T.copy())


@pytest.mark.parametrize("mode", ["baseline", "htree_c6"])
def test_no_stale_plan(mode):
    """frame A, predict, frame B of the same shape and another topology on the same pipeline, predict: B's result is B's.  The
    logits are compared as well as the labels, so the test does not lean on the two frames getting different labels."""
    torch.manual_seed(3)
    cls = HomogeneousNeuralTreeNetwork if MODES[mode][0] else HomogeneousNetwork
    net = cls(6, output_dim=26, conv_block="GraphSAGE", hidden_dim=32, num_layers=3, dropout=0.25).to(DEV).eval()
    a, b = shifted_rooms_frame(0), shifted_rooms_frame(1)
    want = []
    for f in (a, b):
        d = oracle(f, mode)[0].to(DEV)
        with torch.no_grad():
            want.append((net(d).clone(), net.predict(d).clone()))
    assert not torch.equal(want[0][0], want[1][0])  # the two frames are told apart by the model
    pipe = dsg.FramePipeline(DEV, htree=MODES[mode][0], clique_dim=MODES[mode][3], homogeneous=True)
    da, _ = pipe.convert(*a)
    got_a = net.predict(da).clone()
    db, _ = pipe.convert(*b)
    assert da.edge_index is not db.edge_index and da.edge_index.shape == db.edge_index.shape and da.x.shape == db.x.shape
    got_b = net.predict(db).clone()
    with torch.no_grad():
        logits_b = net(db).clone()
    assert torch.equal(got_a, want[0][1]) and torch.equal(got_b, want[1][1]) and torch.equal(logits_b, want[1][0])
    dc, _ = pipe.convert(*b)  # the same frame again: fresh tensor objects, which predict's plan reuse depends on
    for k, t in attributes(dc).items():
        assert t is not getattr(db, k) and torch.equal(t, getattr(db, k)), k


def test_another_stream_is_refused():
    pipe = dsg.FramePipeline(DEV, homogeneous=True)
    first, _ = pipe.convert(*fc.frame((7, 2)))
    with torch.cuda.stream(torch.cuda.Stream(DEV)):
        with pytest.raises(_lib.HydraMPError, match="stream"):
            pipe.convert(*fc.frame((7, 2)))
    got, _ = pipe.convert(*fc.frame((7, 2)))  # back on the pipeline's stream
    assert_same_data(got, oracle(fc.frame((7, 2)), "baseline")[0])
