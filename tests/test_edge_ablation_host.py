"""Host contract of the edge-type and clique ablations (``data.heterogeneous_data_to_homogeneous(removed_edge_type=)``,
``data.remove_edge_types``, ``data.zero_clique_features``): the parity oracles of the derived stores.  Each is checked against a
literal restatement of the reference written here (``mp3d_dataset.py:53-69``: convert without removal, then mask
``edge_type != index``; ``train_Stanford.py:93-99``: ``x[clique rows] = 0``).  No GPU."""
import pytest
import torch

import _store_derive_cases as sc
from hydra_gnn_amd import data as hdata


def same_data(got, want):
    keys = lambda d: [k for k, v in d.__dict__.items() if isinstance(v, torch.Tensor)]
    assert keys(got) == keys(want)
    for k in keys(want):
        g, w = getattr(got, k), getattr(want, k)
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), k


@pytest.mark.parametrize("removed", [sc.OO, sc.RR, sc.OR, sc.RO])
@pytest.mark.parametrize("with_attr", [False, True])
def test_removed_edge_type_is_convert_then_mask(removed, with_attr):
    for g in sc.baseline_graphs(True, ro_edges=True):
        if with_attr:
            g = sc.relative_pos(g)
        want, want_types = hdata.heterogeneous_data_to_homogeneous(sc.clone(g))
        index = list(g.edge_index_dict.keys()).index(removed)
        mask = want.edge_type != index
        n_all = want.edge_index.size(1)
        want.edge_index = want.edge_index[:, mask]
        want.edge_type = want.edge_type[mask]
        if with_attr:
            want.edge_attr = want.edge_attr[mask]
        got, types = hdata.heterogeneous_data_to_homogeneous(sc.clone(g), removed_edge_type=removed)
        assert types == want_types
        same_data(got, want)
        assert hasattr(got, "edge_attr") == with_attr
        # the surviving types keep their numbers, the removed one is gone
        assert index not in got.edge_type.tolist() and got.edge_index.size(1) == n_all - g[removed].edge_index.size(1)
        assert got.edge_index.dtype == torch.int64 and got.edge_index.shape == (2, got.edge_type.numel())


def test_default_is_todays_conversion_and_the_return_stays_a_pair():
    g = sc.baseline_graphs(True, ro_edges=True)[0]
    out = hdata.heterogeneous_data_to_homogeneous(sc.clone(g), removed_edge_type=None)
    assert isinstance(out, tuple) and len(out) == 2
    same_data(out[0], hdata.heterogeneous_data_to_homogeneous(sc.clone(g))[0])


def test_unknown_triple_is_a_value_error():
    g = sc.baseline_graphs(True)[0]
    with pytest.raises(ValueError, match="not an edge type"):
        hdata.heterogeneous_data_to_homogeneous(g, removed_edge_type=("rooms", "rooms_to_places", "places"))
    with pytest.raises(ValueError, match="not an edge type"):
        hdata.remove_edge_types(g, [("rooms", "rooms_to_places", "places")])


def test_remove_edge_types_on_a_typed_graph_keeps_the_type_empty():
    for g in sc.baseline_graphs(True, ro_edges=True):
        g = sc.relative_pos(g)
        before = sc.clone(g)
        assert hdata.remove_edge_types(g, [sc.RR, sc.RO]) is g
        assert g.edge_types == before.edge_types and g.node_types == before.node_types
        for e in (sc.RR, sc.RO):
            assert g[e].edge_index.shape == (2, 0) and g[e].edge_index.dtype == torch.int64
            assert g[e].edge_attr.shape == (0, 3) and g[e].edge_attr.dtype == torch.float32
        for e in (sc.OO, sc.OR):
            assert torch.equal(g[e].edge_index, before[e].edge_index) and torch.equal(g[e].edge_attr, before[e].edge_attr)
        for t in g.node_types:
            assert torch.equal(g[t].x, before[t].x)
    g = sc.baseline_graphs(False)[0]  # no edge_attr: none appears
    hdata.remove_edge_types(g, [sc.RR])
    assert "edge_attr" not in g[sc.RR] and g[sc.RR].edge_index.shape == (2, 0)


@pytest.mark.parametrize("ids", [[0], [1, 2], [5], [0, 1, 2, 3], []])
def test_remove_edge_types_on_a_homogeneous_graph_drops_columns_by_edge_type(ids):
    for g in sc.baseline_graphs(True, ro_edges=True):
        d = sc.homogeneous(sc.relative_pos(g))
        want = sc.clone(d)
        keep = torch.tensor([t not in ids for t in d.edge_type.tolist()], dtype=torch.bool)
        want.edge_index, want.edge_type, want.edge_attr = d.edge_index[:, keep], d.edge_type[keep], d.edge_attr[keep]
        same_data(hdata.remove_edge_types(d, ids), want)


def test_homogeneous_removal_leaves_init_and_pool_edges():
    for g in sc.htree_graphs(True):
        d = sc.homogeneous(g)
        init, pool, n = d.init_edge_index.clone(), d.pool_edge_index.clone(), d.edge_index.size(1)
        first = int(d.edge_type[0])
        hdata.remove_edge_types(d, [first])
        assert torch.equal(d.init_edge_index, init) and torch.equal(d.pool_edge_index, pool)
        assert 0 < d.edge_index.size(1) < n and first not in d.edge_type.tolist()


def test_zero_clique_features_typed_and_homogeneous():
    for g in sc.htree_graphs(True):
        before = sc.clone(g)
        assert any(float(before[t].x.abs().sum()) > 0 for t in ("object-room", "room-room"))  # the mean room position is there
        assert hdata.zero_clique_features(g) is g
        for t in g.node_types:
            if t in ("object-room", "room-room"):
                assert g[t].x.shape == before[t].x.shape and g[t].x.dtype == torch.float32 and not g[t].x.any()
            else:
                assert torch.equal(g[t].x, before[t].x)
        # homogeneous: the rows of the two clique types, literally
        d = sc.homogeneous(sc.clone(before))
        types = [t for t in before.node_types if "x" in before[t]]
        clique = (d.node_type == types.index("object-room")) | (d.node_type == types.index("room-room"))
        want = d.x.clone()
        want[clique] = 0
        x_in = d.x
        hdata.zero_clique_features(d)
        assert torch.equal(d.x, want) and bool(clique.any()) and d.x is not x_in
        # ... which is the conversion of the zeroed typed tree
        assert torch.equal(d.x, sc.homogeneous(sc.clone(g)).x)


def test_zero_clique_features_refuses_a_graph_that_is_no_htree():
    g = sc.baseline_graphs(True)[0]
    with pytest.raises(ValueError, match="not an H-tree"):
        hdata.zero_clique_features(g)
    with pytest.raises(ValueError, match="not an H-tree"):
        hdata.zero_clique_features(sc.homogeneous(sc.clone(g)))
