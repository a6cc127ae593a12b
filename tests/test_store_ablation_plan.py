"""The plans of the ablation derivations, without a device: ``to_homogeneous(removed_edge_type=RO)`` plans no item that reads the
removed type's arrays, and the two new item kinds of ``DerivePlan`` (``compact``: rows compacted by a key vector, ``rows_zero``: rows
zeroed where the key is in a set) lay their words out as ``include/hydra_mp.h`` section 15 says.  The store is built over host
tensors (addresses are plain ints to a plan); nothing is launched."""
import numpy as np
import pytest
import torch

import _store_derive_cases as sc
from hydra_gnn_amd import _lib, store as hstore
from hydra_gnn_amd.store import DerivePlan, GraphStore


@pytest.fixture
def host_store(monkeypatch):
    monkeypatch.setattr(_lib, "require_device", lambda: None)
    return lambda graphs: GraphStore(graphs, "cpu")


def addresses(it):
    return {int(it[w]) for w in (_lib.SD_SRC, _lib.SD_SRC_PTR, _lib.SD_A0, _lib.SD_A1, _lib.SD_A2, _lib.SD_A3) if not isinstance(it[w], tuple)}


@pytest.mark.parametrize("with_attr", [False, True])
def test_to_homogeneous_plans_no_item_that_reads_the_removed_type(host_store, with_attr):
    graphs = sc.baseline_graphs(True, ro_edges=True)
    if with_attr:
        graphs = [sc.relative_pos(g) for g in graphs]
    s = host_store(graphs)
    removed = {s.edge_index[sc.RO].data_ptr(), s.edge_ptr[sc.RO].data_ptr()} | ({s.edge_attr[sc.RO].data.data_ptr()} if with_attr else set())
    full, _ = hstore._plan_to_homogeneous(s)
    plan, parts = hstore._plan_to_homogeneous(s, removed_edge_type=sc.RO)
    assert any(addresses(it) & removed for it in full.items)  # the addresses do identify the type's items ...
    assert not any(addresses(it) & removed for it in plan.items)  # ... and none is left
    per_type = 3 if with_attr else 2  # edges + edge_type fill (+ edge_attr rows)
    assert len(plan.items) == len(full.items) - per_type
    # the other types keep their numbers (the position among the store's edge types: OO, RR, OR, RO)
    assert s.edge_types == [sc.OO, sc.RR, sc.OR, sc.RO]
    edge_type = parts[4]
    fills = [int(it[_lib.SD_A0]) for it in plan.items if it[_lib.SD_KIND] == _lib.SD_FILL and it[_lib.SD_DST] == edge_type.data_ptr()]
    assert fills == [0, 1, 2]
    # and the edge list is as long as the three kept types
    edge_ptr_host = parts[2]["edge_index"]
    want = sum(np.diff(s.edge_ptr_host[e]) for e in (sc.OO, sc.RR, sc.OR))
    assert np.array_equal(np.diff(edge_ptr_host), want) and parts[3]["edge_index"].shape == (2, int(want.sum()))


def test_removed_edge_type_refusals(host_store):
    s = host_store(sc.baseline_graphs(True))
    with pytest.raises(_lib.HydraMPError, match="not an edge type of the store"):
        hstore._plan_to_homogeneous(s, removed_edge_type=("rooms", "rooms_to_places", "places"))
    t = host_store(sc.htree_graphs(True))
    with pytest.raises(_lib.HydraMPError, match="refused on an H-tree store"):
        hstore._plan_to_homogeneous(t, removed_edge_type=t.edge_types[0])


def test_compact_and_rows_zero_items():
    G = 9
    plan = DerivePlan(G)
    off = np.arange(G, dtype=np.int64) * 3
    plan.compact(0x1000, 0x2000, 0x3000, off, 40, 8, 0x4000, 0b101)
    plan.compact(0x1004, 0x2004, 0x3000, off, 40, 12, 0x4000, 1 << 63)  # 4-byte aligned arrays: 4-byte units; bit 63 as an int64 word
    plan.compact(0x1000, 0x2000, 0x3000, off, 0, 8, 0x4000, 1)  # nothing to walk: no item
    plan.rows_zero(0x5000, 0x6000, 0x3000, off, 40, 48, 0x4000, 0b1100)
    plan.rows_zero(0x5004, 0x6000, 0x3000, off, 40, 36, 0x4000, 0b1100)
    a, b, c, d = plan.items
    assert a[_lib.SD_KIND] == b[_lib.SD_KIND] == _lib.SD_COMPACT == 4 and c[_lib.SD_KIND] == d[_lib.SD_KIND] == _lib.SD_ROWS_ZERO == 5
    assert (a[_lib.SD_UNIT], a[_lib.SD_SRC_W], a[_lib.SD_DST_W], a[_lib.SD_A0], a[_lib.SD_A1], a[_lib.SD_N]) == (8, 1, 1, 0x4000, 0b101, 40)
    assert (b[_lib.SD_UNIT], b[_lib.SD_SRC_W], b[_lib.SD_DST_W], b[_lib.SD_A1]) == (4, 3, 3, -(1 << 63))
    assert (c[_lib.SD_UNIT], c[_lib.SD_SRC_W], c[_lib.SD_TAKE], c[_lib.SD_DST_W], c[_lib.SD_SKIP], c[_lib.SD_A1]) == (16, 3, 3, 3, 0, 0b1100)
    assert (d[_lib.SD_UNIT], d[_lib.SD_DST_W]) == (4, 9)
    # a wave per graph: 64 threads' worth of work per graph; a thread per destination unit for rows_zero
    assert plan.work == [G * 64, G * 64, 40 * 3, 40 * 9]
    block, n_blocks = plan.pack(0x10000)
    assert n_blocks == 3 + 3 + 1 + 2 and block.dtype == np.int64
    _, item0, where = plan.layout()
    assert block[item0 + _lib.SD_A1 + _lib.SD_ITEM_WORDS] == -(1 << 63)
    assert block[where[0]:where[0] + G].tolist() == off.tolist()
    with pytest.raises(AssertionError):
        plan.compact(0x1000, 0x2000, 0x3000, off, 40, 8, 0x4000, 1 << 64)  # ids of 64 and above have no bit
