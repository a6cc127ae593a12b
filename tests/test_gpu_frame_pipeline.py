"""``dsg.FramePipeline`` on the device (csrc/frame.hip: one upload, one launch) against the existing conversion path
(``dsg.frame_to_data`` / ``data.compute_relative_pos`` / ``htree.generate_htree``), which stays as it is and is the oracle here:
every tensor of the baseline frame and of the H-tree bit for bit (clique means of more than two rooms within the bound of a
sequential float32 sum -- the existing path's ``index_add_`` has no defined order), equal predictions of three model classes, no
plan carried from one frame to a different one of the same shape, arena growth, and the refusal of a foreign device."""
import numpy as np
import pytest
import torch

import _frame_cases as fc
from hydra_gnn_amd import _lib, dsg, htree
from hydra_gnn_amd.models import HeterogeneousNetwork, HeterogeneousNeuralTreeNetwork

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ["fixture"] + fc.SIZES
_EXISTING, _PIPES = {}, {}


def existing(name, sem=False, relative_pos=False):
    """the existing path's frame, computed once and left unchanged"""
    key = (name, sem, relative_pos)
    if key not in _EXISTING:
        if name == "fixture" and not sem:
            data, _ = dsg.frame_to_data(fc.JSON, device=DEV)
            if relative_pos:
                from hydra_gnn_amd.data import compute_relative_pos
                compute_relative_pos(data)
        else:
            data, _ = fc.existing_frame(fc.frame(name), sem, relative_pos, device=DEV)
        _EXISTING[key] = data
    return _EXISTING[key]


def pipeline(sem=False, relative_pos=False, htree_mode=False):
    key = (sem, relative_pos, htree_mode)
    if key not in _PIPES:
        _PIPES[key] = dsg.FramePipeline(DEV, semantic_table=fc.semantic_table() if sem else None, htree=htree_mode, relative_pos=relative_pos,
                                        clique_dim=6 if htree_mode else None)
    return _PIPES[key]


def assert_same_frame(got, want, skip=()):
    assert got.node_types == want.node_types and got.edge_types == want.edge_types
    for key in want.node_types + want.edge_types:
        assert sorted(got[key].keys()) == sorted(want[key].keys()), key
        for attr, w in want[key].items():
            if (key, attr) in skip:
                continue
            g = getattr(got[key], attr)
            assert g.dtype == w.dtype and g.shape == w.shape and g.is_contiguous() and torch.equal(g, w), (key, attr)


@pytest.mark.parametrize("sem", [False, True], ids=["sem0", "sem300"])
@pytest.mark.parametrize("name", CASES, ids=str)
def test_baseline_parity(name, sem):
    arrays = fc.frame(name)
    got, info = pipeline(sem).convert(*arrays)
    want = existing(name, sem)
    assert_same_frame(got, want)
    assert got["objects"].x.shape[1] == (306 if sem else 6) and got["rooms"].x.shape[1] == 6
    assert info["object_ids"].tolist() == want["objects"].node_ids.cpu().tolist() and info["room_ids"].tolist() == want["rooms"].node_ids.cpu().tolist()
    got, _ = pipeline(sem, relative_pos=True).convert(*arrays)
    assert_same_frame(got, existing(name, sem, relative_pos=True))  # x without its leading xyz, edge_attr on all four edge types
    assert got["objects", "objects_to_objects", "objects"].edge_attr.shape[1] == 3


def test_fixture_info_and_scene_entry():
    exp = np.load(fc.EXP)
    got, info = pipeline().convert_scene(dsg.load_dsg_json(fc.JSON))
    assert_same_frame(got, existing("fixture"))
    assert np.array_equal(info["object_ids"], exp["obj_id"]) and np.array_equal(info["room_ids"], exp["room_id"])
    assert np.array_equal(np.sort(info["dropped_ids"]), exp["dropped_obj_id"])


@pytest.mark.parametrize("sem", [False, True], ids=["sem0", "sem300"])
@pytest.mark.parametrize("name", CASES, ids=str)
def test_htree_parity(name, sem):
    want = htree.generate_htree(existing(name, sem), clique_dim=6)
    got, _ = pipeline(sem, htree_mode=True).convert(*fc.frame(name))
    cliques = [("object-room", "x"), ("room-room", "x")]
    assert_same_frame(got, want, skip=cliques)  # every edge list, the leaf gathers, leaf and virtual x / pos / label
    rpos = want["room_virtual"].pos.cpu().numpy()
    for which, nt in ((2, "object-room"), (3, "room-room")):
        g, w = got[nt].x.cpu().numpy(), want[nt].x.cpu().numpy()
        assert g.shape == w.shape and g.dtype == w.dtype and g.shape[1] == 6 and not g[:, 3:].any()
        for q, members in enumerate(fc.clique_members(want, which)):
            k = len(members)
            if k <= 2:
                assert np.array_equal(g[q, :3], w[q, :3]), (nt, q, k)
                continue
            p = rpos[members].astype(np.float64)
            bound = k * 2.0 ** -24 * np.abs(p).max(0)  # sequential float32 sum of k terms and one division
            assert (np.abs(g[q, :3] - p.mean(0)) <= bound).all(), (nt, q, k, g[q, :3], p.mean(0), bound)


def labels(net, frame):
    return net.predict(frame).clone()


def test_predictions_equal():
    torch.manual_seed(0)
    sage = HeterogeneousNetwork(input_dim_dict={"objects": 6, "rooms": 6}, output_dim=26, conv_block="GraphSAGE", hidden_dim=64, num_layers=3,
                                dropout=0.25).to(DEV).eval()
    gat = HeterogeneousNetwork(input_dim_dict={"objects": 3, "rooms": 3}, output_dim=26, conv_block="GAT_edge", GAT_hidden_dims=[16, 16],
                               GAT_heads=[2, 2, 2], GAT_concats=[True, True, False], dropout=0.25).to(DEV).eval()
    dims = {"object": 6, "room": 6, "object-room": 6, "room-room": 6, "object_virtual": 6, "room_virtual": 6}
    tree = HeterogeneousNeuralTreeNetwork(dims, output_dim=26, conv_block="GraphSAGE", hidden_dim=32, num_layers=3, disable_initialization=True,
                                          dropout=0.25).to(DEV).eval()
    for name in ("fixture", (300, 3)):
        arrays = fc.frame(name)
        want = labels(sage, existing(name))
        assert torch.equal(labels(sage, pipeline().convert(*arrays)[0]), want) and want.numel() == existing(name)["rooms"].x.size(0)
        want = labels(gat, existing(name, relative_pos=True))
        assert torch.equal(labels(gat, pipeline(relative_pos=True).convert(*arrays)[0]), want)
        want = labels(tree, htree.generate_htree(existing(name), clique_dim=6))
        assert torch.equal(labels(tree, pipeline(htree_mode=True).convert(*arrays)[0]), want)


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


def test_no_plan_is_carried_to_a_different_frame_of_the_same_shape():
    from oracle import models as omodels

    torch.manual_seed(3)  # weights under which the CPU oracle gives the two frames different labels in 4 of the 6 rooms
    kw = dict(input_dim_dict={"objects": 6, "rooms": 6}, output_dim=26, conv_block="GraphSAGE", hidden_dim=64, num_layers=3, dropout=0.25)
    net = HeterogeneousNetwork(**kw)
    net.load_state_dict(omodels.HeterogeneousNetwork(**kw).state_dict(), strict=True)
    net = net.to(DEV).eval()
    a, b = shifted_rooms_frame(0), shifted_rooms_frame(1)
    want = [labels(net, fc.existing_frame(f, False, device=DEV)[0]) for f in (a, b)]
    assert not torch.equal(want[0], want[1])  # the two frames are told apart by the model
    pipe = dsg.FramePipeline(DEV)
    fa, _ = pipe.convert(*a)
    got_a = labels(net, fa)
    fb, _ = pipe.convert(*b)
    RO = ("rooms", "rooms_to_objects", "objects")
    assert fa[RO].edge_index is not fb[RO].edge_index and fa[RO].edge_index.shape == fb[RO].edge_index.shape
    assert [fa[t].x.size(0) for t in fa.node_types] == [fb[t].x.size(0) for t in fb.node_types]
    got_b = labels(net, fb)
    assert torch.equal(got_a, want[0]) and torch.equal(got_b, want[1])


def test_arena_growth():
    pipe = dsg.FramePipeline(DEV, semantic_table=fc.semantic_table())
    small, _ = pipe.convert(*fc.frame((7, 2)))
    assert_same_frame(small, existing((7, 2), True))
    before = pipe._arena.numel()
    big, _ = pipe.convert(*fc.frame((300, 3)))
    assert pipe._arena.numel() > before  # the (300, 3) frame with 306-d rows does not fit the first arena
    assert_same_frame(big, existing((300, 3), True))
    again, _ = pipe.convert(*fc.frame((7, 2)))
    assert_same_frame(again, existing((7, 2), True))


def test_a_foreign_device_is_refused_before_anything_is_enqueued(monkeypatch):
    pipe = dsg.FramePipeline(DEV)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 1)
    with pytest.raises(_lib.HydraMPError, match="current device"):
        pipe.convert(*fc.frame((7, 2)))
    assert pipe._arena is None and pipe._d_staging is None  # refused before any buffer or launch
    with pytest.raises(_lib.HydraMPError, match="no CPU fallback"):
        dsg.FramePipeline("cpu")


def test_another_stream_is_refused():
    """one staging buffer and one arena per pipeline are ordered by one stream: a convert under another current stream is refused"""
    pipe = dsg.FramePipeline(DEV)
    pipe.convert(*fc.frame((7, 2)))
    with torch.cuda.stream(torch.cuda.Stream(DEV)):
        with pytest.raises(_lib.HydraMPError, match="stream"):
            pipe.convert(*fc.frame((7, 2)))
    got, _ = pipe.convert(*fc.frame((7, 2)))  # back on the pipeline's stream
    assert_same_frame(got, existing((7, 2)))
