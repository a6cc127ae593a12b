"""Edge-type and clique ablations on the device: ``GraphStore.without_edge_types`` / ``to_homogeneous(removed_edge_type=)`` /
``zero_clique_features`` (csrc/store_derive.hip: the count launch, the ``HMP_SD_COMPACT`` and ``HMP_SD_ROWS_ZERO`` items),
``FramePipeline(remove_room_edges=True)``, and streams over an edge type that is empty in the whole store (csrc/collate.hip).

Every derived store is compared with ``GraphStore`` over the host transform of every graph (``data.remove_edge_types`` /
``data.heterogeneous_data_to_homogeneous(removed_edge_type=)`` / ``data.zero_clique_features``), packed array for packed array and
offset vector for offset vector, with every output pre-filled with 0xA5; the frames with the existing path (``frame_to_data``
arithmetic with ``rooms_to_rooms`` emptied, then ``htree.generate_htree``); training steps bit for bit."""
import numpy as np
import pytest
import torch

import _frame_batch_cases as bc
import _frame_cases as fc
import _store_derive_cases as sc
from hydra_gnn_amd import _lib, data as hdata, dsg, htree, store as hstore
from hydra_gnn_amd.data import Data
from hydra_gnn_amd.models import HeterogeneousNetwork, HomogeneousNetwork, HomogeneousNeuralTreeNetwork
from hydra_gnn_amd.store import HOMO_NODE, GraphStore

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E0 = hstore.homo_edge_type("edge_index")


@pytest.fixture(autouse=True)
def prefilled_outputs(monkeypatch):
    def alloc(shape, dtype, device):
        t = torch.empty(shape, dtype=dtype, device=device)
        if t.numel():
            t.reshape(-1).view(torch.uint8).fill_(0xA5)
        return t

    monkeypatch.setattr(hstore, "_derive_alloc", alloc)


# ---- the compaction kernel on hand-made homogeneous graphs -----------------------------------------------------------------------
# edges per graph: none, one, a full sweep of the wave, one more, two sweeps and one more
EDGE_COUNTS = {1: [129], 9: [0, 1, 64, 65, 129, 3, 0, 64, 2]}
_HAND = {}


def hand_made(G, with_attr, all_type=None):
    """homogeneous ``Data`` with interleaved edge types (``arange % 3``; ``all_type``: one type on every edge) and edges that differ
    column by column, so that a misplaced or repeated column shows"""
    key = (G, with_attr, all_type)
    if key not in _HAND:
        rng = np.random.default_rng(31 + G)
        graphs = []
        for gi, n_e in enumerate(EDGE_COUNTS[G]):
            n = 5 + gi
            d = Data(x=torch.from_numpy(rng.standard_normal((n, 4)).astype(np.float32)),
                     edge_index=torch.from_numpy(np.stack([np.arange(n_e) % n, (np.arange(n_e) * 3 + gi) % n]).astype(np.int64)),
                     edge_type=torch.arange(n_e, dtype=torch.int64) % 3 if all_type is None else torch.full((n_e,), all_type, dtype=torch.int64))
            if with_attr:
                d.edge_attr = torch.from_numpy(rng.standard_normal((n_e, 3)).astype(np.float32))
            d.train_mask = torch.arange(n) % 2 == 0
            d.val_mask, d.test_mask = ~d.train_mask, torch.zeros(n, dtype=torch.bool)
            graphs.append(d)
        _HAND[key] = graphs
    return _HAND[key]


def check_compaction(graphs, ids):
    parent = GraphStore(graphs, DEV)
    got = parent.without_edge_types(ids)
    want = GraphStore([hdata.remove_edge_types(sc.clone(g), ids) for g in graphs], DEV)
    torch.cuda.synchronize()
    sc.assert_same_store(got, want)
    sc.assert_same_store(parent, GraphStore(graphs, DEV))  # the receiver is unchanged
    # unchanged arrays are shared, mask rows are the new store's own
    attrs, p_attrs = got.node_attrs[HOMO_NODE], parent.node_attrs[HOMO_NODE]
    assert attrs["x"].data.data_ptr() == p_attrs["x"].data.data_ptr()
    assert all(attrs[k].data.data_ptr() != p_attrs[k].data.data_ptr() for k in hstore.DEFAULT_MASKS)
    return got


@pytest.mark.parametrize("ids", [[0], [1, 2], [5], [0, 1, 2]], ids=str)
@pytest.mark.parametrize("with_attr", [False, True], ids=["no_attr", "attr3"])
@pytest.mark.parametrize("G", [1, 9])
def test_compaction_equals_the_store_of_the_host_transform(G, with_attr, ids):
    graphs = hand_made(G, with_attr)
    got = check_compaction(graphs, ids)
    n_all = sum(EDGE_COUNTS[G])
    n_kept = int(got.edge_ptr_host[E0][-1])
    assert n_kept == {(5,): n_all, (0, 1, 2): 0}.get(tuple(ids), n_kept) and list(got.edge_rows[E0]) == ["edge_type"] + (["edge_attr"] if with_attr else [])
    if ids == [0]:
        assert 0 < n_kept < n_all


def test_compaction_with_one_type_on_every_edge():
    """whole sweeps kept and whole sweeps dropped: the ballot is all ones / all zeros"""
    check_compaction(hand_made(9, True, all_type=1), [1])
    check_compaction(hand_made(9, True, all_type=1), [0])


def test_waves_stride_over_the_graphs(monkeypatch):
    """one workgroup per item: its four waves walk the nine graphs in three passes (and the other items their rows)"""
    monkeypatch.setattr(hstore.DerivePlan, "MAX_BLOCKS", 1)
    check_compaction(hand_made(9, True), [1])


def test_edge_type_numbers_of_64_and_above_are_refused():
    s = GraphStore(hand_made(1, False), DEV)
    with pytest.raises(_lib.HydraMPError, match=r"outside \[0, 64\)"):
        s.without_edge_types([64])
    with pytest.raises(_lib.HydraMPError, match=r"outside \[0, 64\)"):
        s.without_edge_types([-1])
    with pytest.raises(_lib.HydraMPError, match="edge type numbers"):
        s.without_edge_types([sc.RO])
    sc.assert_same_store(s.without_edge_types([63]), GraphStore(hand_made(1, False), DEV))  # the last bit of the set
    typed = GraphStore(sc.baseline_graphs(True), DEV)
    with pytest.raises(_lib.HydraMPError, match="not an edge type of the store"):
        typed.without_edge_types([2])


# ---- typed removal and the three routes to the homogeneous store without one type -------------------------------------------------
_GRAPHS = {}


def baseline_ro(relpos=False):
    if relpos not in _GRAPHS:
        graphs = sc.baseline_graphs(True, ro_edges=True)
        _GRAPHS[relpos] = [sc.relative_pos(g) for g in graphs] if relpos else graphs
    return _GRAPHS[relpos]


@pytest.mark.parametrize("relpos", [False, True], ids=["plain", "edge_attr"])
@pytest.mark.parametrize("types", [[sc.RR], [sc.RO, sc.RR], [sc.OO, sc.RR, sc.OR, sc.RO]], ids=["RR", "RO_RR", "all"])
def test_typed_removal_equals_the_store_of_the_host_transform(types, relpos):
    graphs = baseline_ro(relpos)
    parent = GraphStore(graphs, DEV)
    got = parent.without_edge_types(types)
    sc.assert_same_store(got, GraphStore([hdata.remove_edge_types(sc.clone(g), types) for g in graphs], DEV))
    sc.assert_same_store(parent, GraphStore(graphs, DEV))
    kept = [e for e in parent.edge_types if e not in types]
    assert all(got.edge_index[e].data_ptr() == parent.edge_index[e].data_ptr() for e in kept)  # shared
    assert all(got.edge_index[e].shape == (2, 0) and not got.edge_ptr_host[e].any() for e in types)


@pytest.mark.parametrize("relpos", [False, True], ids=["plain", "edge_attr"])
def test_three_routes_to_the_store_without_rooms_to_objects_agree(relpos):
    graphs = baseline_ro(relpos)
    s = GraphStore(graphs, DEV)
    index = s.edge_types.index(sc.RO)  # to_homogeneous numbers edge_type by the position among the store's edge types
    assert index == list(graphs[0].edge_index_dict).index(sc.RO) == 3
    a = s.to_homogeneous(removed_edge_type=sc.RO)
    b = s.without_edge_types([sc.RO]).to_homogeneous()
    c = s.to_homogeneous().without_edge_types([index])

    def host(g):
        d, types = hdata.heterogeneous_data_to_homogeneous(sc.clone(g), removed_edge_type=sc.RO)
        d.room_mask = d.node_type == types.index("rooms")
        return d

    want = GraphStore([host(g) for g in graphs], DEV)
    torch.cuda.synchronize()
    for got in (a, b, c):
        sc.assert_same_store(got, want)
    assert index not in a.edge_rows[E0]["edge_type"].data.tolist() and int(a.edge_ptr_host[E0][-1]) > 0
    bc.assert_same_batch(a.collate([4, 1, 1]), want.collate([4, 1, 1]))
    with pytest.raises(_lib.HydraMPError, match="refused on an H-tree store"):
        GraphStore(sc.htree_graphs(True), DEV).to_homogeneous(removed_edge_type=sc.RO)


# ---- clique zeroing -----------------------------------------------------------------------------------------------------------------
def htree_graphs16():
    """H-trees whose rows move in 16-byte units: 8-wide objects (the homogeneous x), 4-wide cliques"""
    if "h16" not in _GRAPHS:
        base = sc.baseline_graphs(True, obj_w=8, room_w=4, counts=[(4, 2), (3, 1), (6, 3)], seed=9)
        for g in base:
            n_o, n_r = g["objects"].num_nodes, g["rooms"].num_nodes
            chain = torch.arange(n_r - 1, dtype=torch.int64)
            g[sc.RR].edge_index = torch.stack([chain, chain + 1]) if n_r > 1 else torch.empty((2, 0), dtype=torch.int64)
            g[sc.RO].edge_index = torch.stack([torch.arange(n_o, dtype=torch.int64) % n_r, torch.arange(n_o, dtype=torch.int64)])
            g[sc.OR].edge_index = g[sc.RO].edge_index.flip(0)
        _GRAPHS["h16"] = [htree.generate_htree(g, clique_dim=4, clique_pos=True) for g in base]
    return _GRAPHS["h16"]


def htree_graphs4():
    if "h4" not in _GRAPHS:
        _GRAPHS["h4"] = sc.htree_graphs(True)
    return _GRAPHS["h4"]


@pytest.mark.parametrize("homogeneous", [False, True], ids=["typed", "homogeneous"])
@pytest.mark.parametrize("unit", [4, 16])
def test_clique_zeroing_equals_the_store_of_the_host_transform(unit, homogeneous):
    graphs = htree_graphs16() if unit == 16 else htree_graphs4()
    if homogeneous:
        graphs = [sc.homogeneous(sc.clone(g)) for g in graphs]
    parent = GraphStore(graphs, DEV)
    x = parent.node_attrs[HOMO_NODE]["x"] if homogeneous else parent.node_attrs["object-room"]["x"]
    assert hstore._unit_of(x.row_bytes, x.data.data_ptr()) == unit
    got = parent.zero_clique_features()
    want = GraphStore([hdata.zero_clique_features(sc.clone(g)) for g in graphs], DEV)
    torch.cuda.synchronize()
    sc.assert_same_store(got, want)
    sc.assert_same_store(parent, GraphStore(graphs, DEV))
    if homogeneous:
        nt, gx, px = got.node_attrs[HOMO_NODE]["node_type"].data, got.node_attrs[HOMO_NODE]["x"].data, x.data
        clique = (nt == 2) | (nt == 3)
        assert bool(px[clique].any()) and not bool(gx[clique].any()) and torch.equal(gx[~clique], px[~clique])
        assert nt.data_ptr() == parent.node_attrs[HOMO_NODE]["node_type"].data.data_ptr() and got.edge_index[E0].data_ptr() == parent.edge_index[E0].data_ptr()
    else:
        assert bool(x.data.any()) and got.node_attrs["object"]["x"].data.data_ptr() == parent.node_attrs["object"]["x"].data.data_ptr()


@pytest.mark.parametrize("width", [9, 8], ids=["unit4", "unit16"])
def test_clique_zeroing_beyond_one_pass_of_the_grid(width):
    """a homogeneous H-tree store whose x has more units than ``MAX_BLOCKS * THREADS`` threads cover in one pass"""
    rng = np.random.default_rng(width)
    rows = 11000 if width == 9 else 44000
    graphs = []
    for gi in range(3):
        n = rows + gi
        node_type = torch.from_numpy(rng.integers(0, 6, n).astype(np.int64))
        graphs.append(Data(x=torch.from_numpy(rng.standard_normal((n, width)).astype(np.float32)), node_type=node_type,
                           room_mask=node_type == 5, object_mask=node_type == 4))
    parent = GraphStore(graphs, DEV)
    x = parent.node_attrs[HOMO_NODE]["x"]
    unit = hstore._unit_of(x.row_bytes, x.data.data_ptr())
    assert unit == (4 if width == 9 else 16)
    assert x.data.numel() * 4 // unit > hstore.DerivePlan.MAX_BLOCKS * hstore.DerivePlan.THREADS
    got = parent.zero_clique_features()
    sc.assert_same_store(got, GraphStore([hdata.zero_clique_features(sc.clone(g)) for g in graphs], DEV))


def test_clique_zeroing_is_refused_on_a_store_that_is_no_htree():
    s = GraphStore(sc.baseline_graphs(True), DEV)
    with pytest.raises(_lib.HydraMPError, match="not an H-tree store"):
        s.zero_clique_features()
    with pytest.raises(_lib.HydraMPError, match="not an H-tree store"):
        s.to_homogeneous().zero_clique_features()


# ---- frames ---------------------------------------------------------------------------------------------------------------------------
FRAME_MODES = {
    "typed": dict(),
    "typed_relpos": dict(relative_pos=True),
    "homog": dict(homogeneous=True),
    "homog_relpos": dict(homogeneous=True, relative_pos=True),
    "htree": dict(htree=True, clique_dim=bc.CLIQUE_DIM),
    "htree_homog": dict(htree=True, clique_dim=bc.CLIQUE_DIM, homogeneous=True),
    "htree_relpos": dict(htree=True, clique_dim=bc.CLIQUE_DIM, htree_relative_pos=True),
    "htree_relpos_homog": dict(htree=True, clique_dim=bc.CLIQUE_DIM, htree_relative_pos=True, homogeneous=True),
}
FRAMES = ["special", (7, 2), "fixture"]
_ORACLE = {}


def oracle(name, mode):
    """the existing path (on the CPU, as ``_frame_batch_cases.cpu_graph``) with ``rooms_to_rooms`` emptied before anything else reads
    it, moved to the device; computed once.  Every clique of an edgeless room layer has one member room, so its mean is exact."""
    if (name, mode) not in _ORACLE:
        kw = FRAME_MODES[mode]
        g, _ = fc.existing_frame(fc.frame(name), False, relative_pos=False)
        hdata.remove_edge_types(g, [sc.RR])
        if kw.get("relative_pos"):
            hdata.compute_relative_pos(g)
        if kw.get("htree"):
            rel = bool(kw.get("htree_relative_pos"))
            g = htree.generate_htree(g, clique_dim=kw["clique_dim"], clique_pos=rel)
            if rel:
                hdata.compute_relative_pos(g)
        if kw.get("homogeneous"):
            g = bc.to_homogeneous(g, bool(kw.get("htree")))
        _ORACLE[name, mode] = g.to(DEV)
    return _ORACLE[name, mode]


def assert_same_graph(got, want):
    if not hasattr(want, "node_types"):
        w = {k: v for k, v in vars(want).items() if isinstance(v, torch.Tensor)}
        g = {k: v for k, v in vars(got).items() if isinstance(v, torch.Tensor)}
        if "y" in w and "y" not in g:  # a frame carries no labels (the H-tree conversion fills -1 where the tree has some)
            del w["y"]
        assert sorted(g) == sorted(w)
        for k, t in w.items():
            assert g[k].dtype == t.dtype and g[k].shape == t.shape and torch.equal(g[k], t), k
        return
    assert got.node_types == want.node_types and got.edge_types == want.edge_types
    for key in want.node_types + want.edge_types:
        assert sorted(got[key].keys()) == sorted(want[key].keys()), key
        for attr, w in want[key].items():
            g = getattr(got[key], attr)
            assert g.dtype == w.dtype and g.shape == w.shape and g.is_contiguous() and torch.equal(g, w), (key, attr)


@pytest.mark.parametrize("mode", list(FRAME_MODES))
def test_frames_without_room_edges_equal_the_existing_path(mode):
    kw = FRAME_MODES[mode]
    pipe = dsg.FramePipeline(DEV, remove_room_edges=True, **kw)
    clones = []
    for name in FRAMES:
        got, _ = pipe.convert(*fc.frame(name))
        want = oracle(name, mode)
        assert_same_graph(got, want)
        clones.append(got.to("cpu"))  # a result is valid until the next convert
    if not kw.get("homogeneous"):  # the room layer is edgeless: rooms_to_rooms empty, no room-room clique
        if kw.get("htree"):
            assert clones[2]["room-room"].x.size(0) == 0 and clones[2]["room", "r_to_rr", "room-room"].edge_index.shape == (2, 0)
        else:
            assert clones[2][sc.RR].edge_index.shape == (2, 0)
    # the flag changes the result of a frame that has room edges
    plain, _ = dsg.FramePipeline(DEV, **kw).convert(*fc.frame("fixture"))
    n_edges = lambda g: g.edge_index.size(1) if kw.get("homogeneous") else sum(g[e].edge_index.size(1) for e in g.edge_types)
    assert n_edges(plain) != n_edges(clones[2])
    # three frames, one launch: the collation of the single results
    batch, infos = pipe.convert_batch([fc.frame(n) for n in FRAMES])
    assert [i["graph"] for i in infos] == [0, 1, 2]
    bc.assert_same_batch(batch, bc.collate(clones, bool(kw.get("homogeneous"))).to(DEV))


@pytest.mark.parametrize("homogeneous", [False, True], ids=["typed", "homogeneous"])
def test_frame_store_without_room_edges(homogeneous):
    fr = bc.frames()
    ys = [bc.class_labels(a, i) for i, a in enumerate(fr)]
    got, infos = GraphStore.from_frames(dsg.FramePipeline(DEV, remove_room_edges=True, homogeneous=homogeneous), fr, ys)
    plain, _ = GraphStore.from_frames(dsg.FramePipeline(DEV), fr, ys)
    assert int(plain.edge_ptr_host[sc.RR][-1]) > 0
    if not homogeneous:
        sc.assert_same_store(got, plain.without_edge_types([sc.RR]))
        assert got.edge_index[sc.RR].shape == (2, 0) and not got.edge_ptr_host[sc.RR].any()
        return
    want = plain.without_edge_types([sc.RR]).to_homogeneous()
    for k in ("x", "node_type", "room_mask", "y"):
        sc.assert_same_value(got.node_attrs[HOMO_NODE][k], want.node_attrs[HOMO_NODE][k], k)
    sc.assert_same_value(got.edge_index[E0], want.edge_index[E0], "edge_index")
    sc.assert_same_value(got.edge_ptr_host[E0], want.edge_ptr_host[E0], "edge_ptr_host")
    sc.assert_same_value(got.edge_rows[E0]["edge_type"], want.edge_rows[E0]["edge_type"], "edge_type")


# ---- end to end: training steps ---------------------------------------------------------------------------------------------------------
GAT = dict(GAT_hidden_dims=[16], GAT_heads=[2, 2], GAT_concats=[True, False])
IDS = [[4, 0, 2], [1, 3]]


def stream_steps(store, make_net, label_type, ids_list):
    torch.manual_seed(0)
    net = make_net().to(DEV)
    net.train()
    step = net.train_step(lr=0.004, weight_decay=0.001, ignored_label=25, seed=3, use_graph=False)
    stream = store.stream(net, 3, label_type, ignored_label=25) if store.homogeneous else store.stream(net, 3, label_type)
    losses = []
    for ids in ids_list:
        step.run(stream.next(ids))
        losses.append(np.float64(step.loss()).tobytes())
    torch.cuda.synchronize()
    return losses, net.native().flat_params().clone()


def collated_steps(graphs, make_net, label_type, ids_list):
    torch.manual_seed(0)
    net = make_net().to(DEV)
    net.train()
    step = net.train_step(lr=0.004, weight_decay=0.001, ignored_label=25, seed=3, use_graph=False)
    losses = []
    for ids in ids_list:
        b = hdata.collate([graphs[i] for i in ids]).to(DEV)
        step(b, b[label_type].y)
        losses.append(np.float64(step.loss()).tobytes())
    torch.cuda.synchronize()
    return losses, net.native().flat_params().clone()


def assert_same_steps(got, want):
    assert got[0] == want[0] and all(np.isfinite(np.frombuffer(b, dtype=np.float64)[0]) for b in got[0])
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))


def test_sage_steps_on_a_store_without_room_edges_equal_host_collated_batches():
    """``rooms_to_rooms`` is empty in the whole store: the stream collates it all the same (no source array, no workgroup)"""
    graphs = baseline_ro()
    make = lambda: HeterogeneousNetwork(input_dim_dict={"objects": sc.OBJ_W, "rooms": sc.ROOM_W}, output_dim=15, conv_block="GraphSAGE",
                                        hidden_dim=16, num_layers=2, dropout=0.25)
    store = GraphStore(graphs, DEV).without_edge_types([sc.RR])
    host = [hdata.remove_edge_types(sc.clone(g), [sc.RR]) for g in graphs]
    got = stream_steps(store, make, "rooms", IDS)
    assert_same_steps(got, collated_steps(host, make, "rooms", IDS))
    assert_same_steps(got, stream_steps(GraphStore(host, DEV), make, "rooms", IDS))  # a store built from noRE graphs streams too


def test_sage_steps_on_a_frame_store_without_room_edges():
    fr = bc.frames()
    ys = [bc.class_labels(a, i) for i, a in enumerate(fr)]
    pipe = dsg.FramePipeline(DEV, remove_room_edges=True)
    store, _ = GraphStore.from_frames(pipe, fr, ys)
    host, _ = bc.single_frame_clones(dsg.FramePipeline(DEV, remove_room_edges=True), fr, ys)
    make = lambda: HeterogeneousNetwork(input_dim_dict={"objects": 6, "rooms": 6}, output_dim=26, conv_block="GraphSAGE", hidden_dim=16,
                                        num_layers=2, dropout=0.25)
    assert_same_steps(stream_steps(store, make, "rooms", IDS), collated_steps(host, make, "rooms", IDS))


def test_gat_steps_on_the_homogeneous_store_without_rooms_to_objects():
    graphs = baseline_ro()
    make = lambda: HomogeneousNetwork(input_dim=sc.OBJ_W, output_dim=15, conv_block="GAT", dropout=0.25, **GAT)

    def host(g):
        d, types = hdata.heterogeneous_data_to_homogeneous(sc.clone(g), removed_edge_type=sc.RO)
        d.room_mask = d.node_type == types.index("rooms")
        return d

    got = stream_steps(GraphStore(graphs, DEV).to_homogeneous(removed_edge_type=sc.RO), make, HOMO_NODE, IDS)
    assert_same_steps(got, stream_steps(GraphStore([host(g) for g in graphs], DEV), make, HOMO_NODE, IDS))
    # the ablation changes what the model sees
    assert got[0] != stream_steps(GraphStore(graphs, DEV).to_homogeneous(), make, HOMO_NODE, IDS)[0]


def test_htree_gat_steps_on_the_zero_clique_homogeneous_store():
    graphs = htree_graphs4()
    make = lambda: HomogeneousNeuralTreeNetwork(input_dim=sc.OBJ_W, output_dim=15, conv_block="GAT", dropout=0.25, disable_initialization=True, **GAT)
    ids = [[3, 0, 2], [1, 3]]
    got = stream_steps(GraphStore(graphs, DEV).to_homogeneous().zero_clique_features(), make, HOMO_NODE, ids)
    want = stream_steps(GraphStore([hdata.zero_clique_features(sc.homogeneous(sc.clone(g))) for g in graphs], DEV), make, HOMO_NODE, ids)
    assert_same_steps(got, want)
    typed = stream_steps(GraphStore(graphs, DEV).zero_clique_features().to_homogeneous(), make, HOMO_NODE, ids)  # the typed route
    assert_same_steps(typed, want)
