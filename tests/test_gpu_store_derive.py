"""Derived stores on the device: ``GraphStore.with_relative_pos`` / ``to_homogeneous`` / ``remove_last_features`` (one
``hmp_store_derive`` launch each, csrc/store_derive.hip) against ``GraphStore`` over the host transform of every graph
(``data.compute_relative_pos``, ``data.heterogeneous_data_to_homogeneous`` / ``heterogeneous_htree_to_homogeneous``, the reference's
``remove_last_features``).  Every packed array, offset vector (device and host) and name list is compared bit for bit, with every
output of a derive pre-filled with 0xA5 so that an element the launch never writes cannot pass by luck.  The same transforms are
cross-checked against the independent frame kernel (``GraphStore.from_frames`` in each mode), and training steps on a derived
store equal those on the oracle store bit for bit.

The typed H-tree frame store (``FramePipeline(htree=True)``) carries no ``pos`` on the clique types, so ``with_relative_pos`` refuses it
(``test_frame_htree_store_without_clique_pos_is_refused``) and the ``htree_relative_pos`` pair is compared on a ``clique_pos`` H-tree store
built from host graphs instead (``test_htree_*``)."""
import numpy as np
import pytest
import torch

import _frame_batch_cases as bc
import _store_derive_cases as sc
from hydra_gnn_amd import _lib, dsg, store as hstore, workloads
from hydra_gnn_amd.models import HeterogeneousNetwork, HomogeneousNetwork, HomogeneousNeuralTreeNetwork
from hydra_gnn_amd.store import HOMO_NODE, GraphStore

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def prefilled_outputs(monkeypatch):
    def alloc(shape, dtype, device):
        t = torch.empty(shape, dtype=dtype, device=device)
        if t.numel():
            t.reshape(-1).view(torch.uint8).fill_(0xA5)
        return t

    monkeypatch.setattr(hstore, "_derive_alloc", alloc)


# name -> (store method chain, host transform chain)
TRANSFORMS = {
    "relpos": (lambda s: s.with_relative_pos(), lambda g: sc.relative_pos(g)),
    "homog": (lambda s: s.to_homogeneous(), lambda g: sc.homogeneous(g)),
    "remove3": (lambda s: s.remove_last_features(3), lambda g: sc.remove_last_features(g, 3)),
    "remove6_rooms_to_width0": (lambda s: s.remove_last_features(6), lambda g: sc.remove_last_features(g, 6)),
    "remove7_rooms_kept": (lambda s: s.remove_last_features(7), lambda g: sc.remove_last_features(g, 7)),
    "relpos_homog": (lambda s: s.with_relative_pos().to_homogeneous(), lambda g: sc.homogeneous(sc.relative_pos(g))),
    "relpos_remove2": (lambda s: s.with_relative_pos().remove_last_features(2), lambda g: sc.remove_last_features(sc.relative_pos(g), 2)),
    "homog_remove4": (lambda s: s.to_homogeneous().remove_last_features(4), lambda g: sc.remove_last_features(sc.homogeneous(g), 4)),
    "relpos_homog_remove2": (lambda s: s.with_relative_pos().to_homogeneous().remove_last_features(2),
                             lambda g: sc.remove_last_features(sc.homogeneous(sc.relative_pos(g)), 2)),
}
_GRAPHS = {}


def graphs_of(kind):
    if kind not in _GRAPHS:
        _GRAPHS[kind] = {"baseline_y": lambda: sc.baseline_graphs(True), "baseline": lambda: sc.baseline_graphs(False),
                         "baseline_ro": lambda: sc.baseline_graphs(True, ro_edges=True),
                         "wide16": lambda: sc.baseline_graphs(True, obj_w=8, room_w=4),  # rows that move in 16-byte units
                         "htree_y": lambda: sc.htree_graphs(True), "htree": lambda: sc.htree_graphs(False)}[kind]()
    return _GRAPHS[kind]


def check(kind, name):
    graphs = graphs_of(kind)
    derive, host = TRANSFORMS[name]
    parent = GraphStore(graphs, DEV)
    got = derive(parent)
    want = GraphStore([host(sc.clone(g)) for g in graphs], DEV)
    torch.cuda.synchronize()
    sc.assert_same_store(got, want)
    sc.assert_same_store(parent, GraphStore(graphs, DEV))  # the receiver is unchanged
    assert len(got) == len(graphs) == got.n_graphs
    return parent, got, want


@pytest.mark.parametrize("name", list(TRANSFORMS))
@pytest.mark.parametrize("kind", ["baseline_y", "baseline"])
def test_baseline_store_equals_the_store_of_the_host_transform(kind, name):
    parent, got, want = check(kind, name)
    if name == "homog":
        assert got.homo_keys == ["x", "node_type", "edge_index", "edge_type"] + (["y"] if kind == "baseline_y" else []) + ["room_mask"]
        b = got.collate([4, 1, 1])
        bc.assert_same_batch(b, want.collate([4, 1, 1]))
    if name == "relpos":  # arrays that do not change are shared with the parent
        assert got.node_attrs["rooms"]["pos"].data.data_ptr() == parent.node_attrs["rooms"]["pos"].data.data_ptr()
        assert got.edge_index[sc.OO].data_ptr() == parent.edge_index[sc.OO].data_ptr()
        assert got.edge_attr[sc.RO].data.shape == (0, 3)  # the edge type that is empty in every graph


@pytest.mark.parametrize("name", ["homog", "remove3", "remove6_rooms_to_width0", "homog_remove4", "relpos_homog"])
def test_rows_that_move_in_16_byte_units(name):
    check("wide16", name)


@pytest.mark.parametrize("name", ["relpos", "homog", "remove3", "relpos_homog", "relpos_homog_remove2"])
@pytest.mark.parametrize("kind", ["htree_y", "htree"])
def test_htree_store_equals_the_store_of_the_host_transform(kind, name):
    parent, got, want = check(kind, name)
    if name == "relpos_homog":
        keys = ["x", "node_type", "edge_index", "edge_type"] + (["y"] if kind == "htree_y" else []) + ["edge_attr", "init_edge_index",
                                                                                                      "pool_edge_index", "room_mask", "object_mask"]
        assert got.homo_keys == keys and list(got.edge_rows[hstore.homo_edge_type("edge_index")]) == ["edge_type", "edge_attr"]
        bc.assert_same_batch(got.collate([2, 0, 3]), want.collate([2, 0, 3]))
        if kind == "htree_y":  # the clique rows, which have no labels, carry -1
            y, nt = got.node_attrs[HOMO_NODE]["y"].data, got.node_attrs[HOMO_NODE]["node_type"].data
            assert bool((y[(nt == 2) | (nt == 3)] == -1).all()) and bool((y[(nt == 4) | (nt == 5)] >= 0).all())


@pytest.mark.parametrize("name", ["relpos", "homog", "relpos_homog", "remove300"])
def test_items_of_many_workgroups_and_the_grid_stride(name):
    """40 MP3D-like graphs (about 4000 nodes, 306-wide objects): an ``x`` item has more destination units than
    ``DerivePlan.MAX_BLOCKS`` workgroups cover in one pass, the edge items span several workgroups"""
    if "big" not in _GRAPHS:
        rng = np.random.Generator(np.random.PCG64(21))
        _GRAPHS["big"] = [workloads.mp3d_like_graph(rng) for _ in range(40)]
    graphs = _GRAPHS["big"]
    n_obj = sum(g["objects"].num_nodes for g in graphs)
    assert n_obj * 303 > hstore.DerivePlan.MAX_BLOCKS * hstore.DerivePlan.THREADS and graphs[0]["objects"].x.size(1) == 306
    derive, host = TRANSFORMS[name] if name != "remove300" else (lambda s: s.remove_last_features(300), lambda g: sc.remove_last_features(g, 300))
    got = derive(GraphStore(graphs, DEV))
    sc.assert_same_store(got, GraphStore([host(sc.clone(g)) for g in graphs], DEV))


def test_a_derived_store_owns_its_mask_rows():
    graphs = [sc.clone(g) for g in graphs_of("baseline_y")]
    for g in graphs:
        for t in ("objects", "rooms"):
            n = g[t].num_nodes
            g[t].train_mask, g[t].val_mask, g[t].test_mask = torch.arange(n) % 3 == 0, torch.arange(n) % 3 == 1, torch.arange(n) % 3 == 2
    parent = GraphStore(graphs, DEV)
    for derive in (lambda s: s.with_relative_pos(), lambda s: s.remove_last_features(3)):
        got = derive(parent)
        for t in ("objects", "rooms"):
            for k in hstore.DEFAULT_MASKS:
                a, b = got.node_attrs[t][k].data, parent.node_attrs[t][k].data
                assert a.data_ptr() != b.data_ptr() and a.dtype == torch.bool and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
            assert got.node_attrs[t]["y"].data.data_ptr() == parent.node_attrs[t]["y"].data.data_ptr()


# ---- the independent frame kernel ---------------------------------------------------------------------------------------------
_FRAME_STORES = {}


def frame_store(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _FRAME_STORES:
        fr = bc.frames()
        ys = [bc.class_labels(a, i) for i, a in enumerate(fr)]
        _FRAME_STORES[key] = GraphStore.from_frames(dsg.FramePipeline(DEV, **kw), fr, ys)[0]
    return _FRAME_STORES[key]


def assert_same_named_arrays(got, want):
    """array by name for the names both homogeneous stores hold, and every offset vector"""
    common = [k for k in want.homo_keys if k in got.homo_keys]
    assert {"x", "edge_index", "node_type", "room_mask"} <= set(common), (got.homo_keys, want.homo_keys)
    e0 = hstore.homo_edge_type("edge_index")
    for k in common:
        if "index" in k:
            e = hstore.homo_edge_type(k)
            sc.assert_same_value(got.edge_index[e], want.edge_index[e], k)
            sc.assert_same_value(got.edge_ptr[e], want.edge_ptr[e], k)
            sc.assert_same_value(got.edge_ptr_host[e], want.edge_ptr_host[e], k)
        elif k in ("edge_attr", "edge_type"):
            sc.assert_same_value(got.edge_rows[e0][k], want.edge_rows[e0][k], k)
        else:
            sc.assert_same_value(got.node_attrs[HOMO_NODE][k], want.node_attrs[HOMO_NODE][k], k)
    sc.assert_same_value(got.node_counts, want.node_counts, "node_counts")


def test_frames_with_relative_pos():
    sc.assert_same_store(frame_store().with_relative_pos(), frame_store(relative_pos=True))


def test_frames_to_homogeneous():
    assert_same_named_arrays(frame_store().to_homogeneous(), frame_store(homogeneous=True))
    assert_same_named_arrays(frame_store(relative_pos=True).to_homogeneous(), frame_store(homogeneous=True, relative_pos=True))
    assert_same_named_arrays(frame_store().with_relative_pos().to_homogeneous(), frame_store(homogeneous=True, relative_pos=True))


def test_frames_htree_to_homogeneous():
    kw = dict(htree=True, clique_dim=bc.CLIQUE_DIM)
    assert_same_named_arrays(frame_store(**kw).to_homogeneous(), frame_store(homogeneous=True, **kw))
    assert_same_named_arrays(frame_store(htree_relative_pos=True, **kw).to_homogeneous(),
                             frame_store(homogeneous=True, htree_relative_pos=True, **kw))


def test_frame_htree_store_without_clique_pos_is_refused():
    typed = frame_store(htree=True, clique_dim=bc.CLIQUE_DIM)
    assert "pos" not in typed.node_attrs["object-room"]  # the typed H-tree frames carry no clique positions
    with pytest.raises(_lib.HydraMPError, match="'object-room'.*has no positions 'pos'"):
        typed.with_relative_pos()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_attribute():
    graphs = graphs_of("baseline_y")
    s = GraphStore(graphs, DEV)
    with pytest.raises(_lib.HydraMPError, match="already holds 'edge_attr'"):
        s.with_relative_pos().with_relative_pos()
    with pytest.raises(_lib.HydraMPError, match="typed store"):
        s.to_homogeneous().with_relative_pos()
    with pytest.raises(_lib.HydraMPError, match="homogeneous already"):
        s.to_homogeneous().to_homogeneous()
    with pytest.raises(_lib.HydraMPError, match="dim must be positive"):
        s.remove_last_features(0)
    no_pos = [sc.clone(g) for g in graphs]
    for g in no_pos:
        del g["rooms"].pos
    with pytest.raises(_lib.HydraMPError, match="'rooms'.*no positions 'pos'"):
        GraphStore(no_pos, DEV).with_relative_pos()
    with pytest.raises(_lib.HydraMPError, match="'x' of node type 'rooms' is 2 wide"):
        GraphStore(_narrow_rooms(graphs), DEV).with_relative_pos()
    places = [sc.clone(g) for g in graphs]
    for g in places:
        g["places"].num_nodes = 3
        g["places", "p_to_r", "rooms"].edge_index = torch.zeros((2, 1), dtype=torch.int64)
    with pytest.raises(_lib.HydraMPError, match="touches node type 'places', which has no features 'x'"):
        GraphStore(places, DEV).to_homogeneous()
    with pytest.raises(_lib.HydraMPError, match="node type 'places' has no features 'x'"):
        GraphStore(places, DEV).with_relative_pos()
    both = [sc.clone(g) for g in graphs_of("htree_y")]
    for g in both:
        g["object_virtual", "ov_to_rv", "room_virtual"].edge_index = torch.zeros((2, 1), dtype=torch.int64)
    with pytest.raises(_lib.HydraMPError, match="virtual node type at both ends"):
        GraphStore(both, DEV).to_homogeneous()


def _narrow_rooms(graphs):
    out = [sc.clone(g) for g in graphs]
    for g in out:
        g["rooms"].x = g["rooms"].x[:, :2].contiguous()
    return out


def test_node_types_without_x_stay_out_of_the_homogeneous_result():
    graphs = [sc.clone(g) for g in graphs_of("baseline_y")]
    for g in graphs:
        g["places"].num_nodes = 3
    got = GraphStore(graphs, DEV).to_homogeneous()
    sc.assert_same_store(got, GraphStore([sc.homogeneous(sc.clone(g)) for g in graphs], DEV))


# ---- end to end: training steps on a derived store ----------------------------------------------------------------------------
GAT = dict(GAT_hidden_dims=[16], GAT_heads=[2, 2], GAT_concats=[True, False])


def two_steps(store, make_net, label_type, ids_list):
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


@pytest.mark.parametrize("case", ["hetero_gat_edge", "homog_sage", "homog_htree_gat"])
def test_training_steps_on_a_derived_store_equal_the_oracle_store(case):
    if case == "hetero_gat_edge":
        graphs, (derive, host) = graphs_of("baseline_ro"), TRANSFORMS["relpos"]
        make = lambda: HeterogeneousNetwork(input_dim_dict={"objects": sc.OBJ_W - 3, "rooms": sc.ROOM_W - 3}, output_dim=15,
                                            conv_block="GAT_edge", dropout=0.25, **GAT)
        label_type, ids = "rooms", [[4, 0, 2], [1, 3]]
    elif case == "homog_sage":
        graphs, (derive, host) = graphs_of("baseline_y"), TRANSFORMS["homog"]
        make = lambda: HomogeneousNetwork(input_dim=sc.OBJ_W, output_dim=15, conv_block="GraphSAGE", hidden_dim=16, num_layers=2, dropout=0.25)
        label_type, ids = HOMO_NODE, [[4, 0, 2], [1, 3]]
    else:
        graphs, (derive, host) = graphs_of("htree_y"), TRANSFORMS["homog"]
        make = lambda: HomogeneousNeuralTreeNetwork(input_dim=sc.OBJ_W, output_dim=15, conv_block="GAT", dropout=0.25,
                                                    disable_initialization=True, **GAT)
        label_type, ids = HOMO_NODE, [[3, 0, 2], [1, 3]]
    got = two_steps(derive(GraphStore(graphs, DEV)), make, label_type, ids)
    want = two_steps(GraphStore([host(sc.clone(g)) for g in graphs], DEV), make, label_type, ids)
    assert got[0] == want[0] and all(np.isfinite(np.frombuffer(b, dtype=np.float64)[0]) for b in got[0])
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
