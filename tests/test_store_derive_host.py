"""Host side of the derived stores and the node split (hydra_gnn_amd/store.py), without a device:

* ``plan_concat``: the offsets of the per-graph concatenation of node types / edge types against
  ``data.heterogeneous_data_to_homogeneous`` per graph followed by the store's (and ``data.collate_homogeneous``'s) concatenation;
* ``DerivePlan``: units, workgroup prefixes, the group table and its two-level lookup, offset vectors behind the item table;
* ``node_split_assignment`` against a restatement of reference ``Stanford3DSG_dataset.py:462-492`` and one committed vector;
* the restated split (``tests/_node_split_reference.py``, the oracle of the GPU tests) against masks recorded from the reference's
  OWN ``generate_node_split`` (``tests/golden/node_split_reference.npz``, written by ``tests/golden/make_node_split_fixture.py``: the
  reference module imports with stand-ins for ``torch_geometric``, so its parity is pinned, on all four data types).
"""
import os

import numpy as np
import pytest
import torch

import _node_split_reference as nsr
import _store_derive_cases as sc
from hydra_gnn_amd import _lib, data as hdata, store
from hydra_gnn_amd.data import Data, HeteroData

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "node_split_reference.npz")


def test_plan_concat_lays_out_what_the_host_conversion_concatenates():
    graphs = sc.baseline_graphs()
    homog = [sc.homogeneous(sc.clone(g)) for g in graphs]
    types = graphs[0].node_types
    width = max(sc.OBJ_W, sc.ROOM_W)
    node_ptr, inside, node_dst = store.plan_concat([[g[t].num_nodes for g in graphs] for t in types])
    assert node_ptr.dtype == np.int64 and node_ptr.tolist() == np.concatenate([[0], np.cumsum([d.num_nodes for d in homog])]).tolist()
    x = np.full((int(node_ptr[-1]), width), np.nan, dtype=np.float32)
    node_type = np.full(int(node_ptr[-1]), -7, dtype=np.int64)
    for i, t in enumerate(types):
        for gi, g in enumerate(graphs):
            n = g[t].num_nodes
            assert inside[i][gi] == sum(g[u].num_nodes for u in types[:i])
            assert np.isnan(x[node_dst[i][gi]:node_dst[i][gi] + n]).all()  # written once
            x[node_dst[i][gi]:node_dst[i][gi] + n] = 0
            x[node_dst[i][gi]:node_dst[i][gi] + n, :g[t].x.size(1)] = g[t].x.numpy()
            node_type[node_dst[i][gi]:node_dst[i][gi] + n] = i
    assert np.array_equal(x, torch.cat([d.x for d in homog]).numpy())
    assert np.array_equal(node_type, torch.cat([d.node_type for d in homog]).numpy())
    edge_types = graphs[0].edge_types
    eptr, _, edst = store.plan_concat([[g[e].edge_index.size(1) for g in graphs] for e in edge_types])
    assert eptr.tolist() == np.concatenate([[0], np.cumsum([d.edge_index.size(1) for d in homog])]).tolist()
    local = np.full((2, int(eptr[-1])), -1, dtype=np.int64)
    edge_type = np.full(int(eptr[-1]), -1, dtype=np.int64)
    for j, e in enumerate(edge_types):
        for gi, g in enumerate(graphs):
            ei = g[e].edge_index.numpy()
            sl = slice(int(edst[j][gi]), int(edst[j][gi]) + ei.shape[1])
            assert (local[:, sl] == -1).all()
            local[0, sl] = ei[0] + inside[types.index(e[0])][gi]
            local[1, sl] = ei[1] + inside[types.index(e[2])][gi]
            edge_type[sl] = j
    assert (local >= 0).all()
    assert np.array_equal(local, torch.cat([d.edge_index for d in homog], dim=1).numpy())  # the store keeps graph-local lists
    assert np.array_equal(edge_type, torch.cat([d.edge_type for d in homog]).numpy())
    shifted = local + np.repeat(node_ptr[:-1], np.diff(eptr))[None, :]
    assert np.array_equal(shifted, hdata.collate_homogeneous(homog).edge_index.numpy())


def lookup(block, n_items, wg):
    """the kernel's two-level item lookup for workgroup ``wg``: two 64-lane loads, two ballots; tail lanes read INT64_MAX"""
    big = np.iinfo(np.int64).max
    n_groups = (n_items + 63) // 64
    items = block[(n_groups + 1) & ~1:]
    lanes = np.arange(64)
    g0 = np.where(lanes < n_groups, block[np.minimum(lanes, n_groups - 1)], big)
    gi = int((g0 <= wg).sum()) - 1
    assert gi >= 0 and bool(np.all((g0 <= wg)[:gi + 1]))
    it = gi * 64 + lanes
    b0 = np.where(it < n_items, items[np.minimum(it, n_items - 1) * _lib.SD_ITEM_WORDS + _lib.SD_BLOCK0], big)
    hit = b0 <= wg
    assert bool(np.all(hit[:int(hit.sum())]))
    return gi * 64 + int(hit.sum()) - 1


def test_derive_plan_units_prefixes_groups_and_vectors():
    G = 3
    plan = store.DerivePlan(G)
    off = np.array([0, 4, 9], dtype=np.int64)
    plan.rows(0x1000, 0x2000, 0x3000, off, 10, 32, 0, 16, 16)       # every width and address a multiple of 16
    plan.rows(0x1000, 0x2000, 0x3000, off, 10, 36, 12, 24, 24)      # x[:, 3:] of a 9-wide float row
    plan.rows(0x1004, 0x2000, 0x3000, off, 10, 32, 0, 16, 16)       # a 4-byte aligned source
    plan.rows(0x1000, 0x2000, 0x3000, off, 10, 1, 0, 1, 1)          # a mask row
    plan.rows(0x1000, 0x2000, 0x3000, off, 0, 36, 12, 24, 24)       # no rows: no item
    plan.rows(0x1000, 0x2000, 0x3000, off, 10, 12, 12, 0, 0)        # nothing left of the row: no item
    assert [it[_lib.SD_UNIT] for it in plan.items] == [16, 4, 4, 1]
    assert [(it[_lib.SD_SRC_W], it[_lib.SD_SKIP], it[_lib.SD_TAKE], it[_lib.SD_DST_W]) for it in plan.items] == [
        (2, 0, 1, 1), (9, 3, 6, 6), (8, 0, 4, 4), (1, 0, 1, 1)]
    assert len(plan.vectors) == 1  # equal offset vectors are stored once
    plan.fill(0x2000, 0x3000, off + 1, 300000, -1, 8)               # more work than MAX_BLOCKS workgroups: capped, grid-stride
    for k in range(70):                                             # a second group
        plan.edges(0x4000, 0x5000, 0x3000, off, 256 * (k % 3) + 1, off, off + 2, 999)
    plan.relpos(0x4000, 0x6000, 0x3000, 77, 0x7000, 0x7100, 0x3000, 0x3100)
    n = len(plan.items)
    assert n == 4 + 1 + 70 + 1
    base = 1 << 20
    block, n_blocks = plan.pack(base)
    words, item0, where = plan.layout()
    assert block.dtype == np.int64 and block.size == words and item0 == 2 and all(w % 2 == 0 for w in where)
    want_blocks = [min(-(-w // 256), plan.MAX_BLOCKS) for w in plan.work]
    assert want_blocks[4] == plan.MAX_BLOCKS and n_blocks == sum(want_blocks)
    items = block[item0:item0 + n * _lib.SD_ITEM_WORDS].reshape(n, _lib.SD_ITEM_WORDS)
    assert items[:, _lib.SD_BLOCK0].tolist() == np.concatenate([[0], np.cumsum(want_blocks)[:-1]]).tolist()
    assert block[0] == 0 and block[1] == items[64, _lib.SD_BLOCK0]
    for wg in list(range(0, n_blocks, 37)) + [n_blocks - 1] + items[:, _lib.SD_BLOCK0].tolist():
        ii = lookup(block, n, wg)
        assert items[ii, _lib.SD_BLOCK0] <= wg < items[ii, _lib.SD_BLOCK0] + want_blocks[ii]
    # vector fields hold addresses inside the block, and the block holds the vectors there
    for it, vec in ((items[0], off), (items[4], off + 1)):
        at = (int(it[_lib.SD_DST_OFF]) - base) // 8
        assert (int(it[_lib.SD_DST_OFF]) - base) % 16 == 0 and block[at:at + G].tolist() == vec.tolist()
    e = items[5]
    assert block[(int(e[_lib.SD_A1]) - base) // 8:][:G].tolist() == (off + 2).tolist() and e[_lib.SD_A3] == 999 and e[_lib.SD_KIND] == _lib.SD_EDGES
    assert items[-1, _lib.SD_KIND] == _lib.SD_RELPOS and items[-1, _lib.SD_A2] == 0x3000
    with pytest.raises(AssertionError):
        plan.rows(0x1000, 0x2000, 0x3000, off, 10, 12, 8, 8, 8)     # reads past the source row


CASES = [(23, (0.5, 0.2, 0.3), 0), (23, (0.4, 0.2, 0.2), 3), (23, (0.5, 0.2, None), 0), (101, (0.7, 0.1, 0.2), 1)]


@pytest.mark.parametrize("total,ratios,seed", CASES)
def test_node_split_assignment_is_the_reference_list(total, ratios, seed):
    got = store.node_split_assignment(total, ratios, seed)
    assert got.dtype == np.int8 and got.shape == (total,)
    assert got.tolist() == nsr.assignment_list(total, *ratios, seed=seed)
    train, val, test = ratios
    rest = test is None
    test = 1 - train - val if rest else test
    assert int((got == 1).sum()) == round(total * train) and int((got == 2).sum()) == round(total * val)
    if train + val + test == 1:
        assert int((got == 0).sum()) == 0 and int((got == 3).sum()) == total - round(total * train) - round(total * val)
    else:
        assert int((got == 3).sum()) == round(total * test) and int((got == 0).sum()) > 0


def test_node_split_assignment_committed_vector():
    want = [3, 3, 1, 2, 1, 1, 1, 3, 1, 1, 3, 1, 3, 1, 1, 1, 3, 2, 2, 1, 1, 2, 2]
    assert store.node_split_assignment(23, (0.5, 0.2, 0.3), 0).tolist() == want


def _fixture_graphs(data_type, counts, extra):
    out = []
    for n_obj, n_room in counts:
        if data_type.startswith("heterogeneous"):
            a, b = ("objects", "rooms") if data_type == "heterogeneous" else ("object_virtual", "room_virtual")
            d = HeteroData()
            d[a].x, d[b].x = torch.zeros(n_obj, 1), torch.zeros(n_room, 1)
        elif data_type == "homogeneous":
            d = Data(x=torch.zeros(n_obj + n_room, 1))
        else:
            n = extra + n_obj + extra + n_room + 1
            d = Data(x=torch.zeros(n, 1), object_mask=torch.zeros(n, dtype=torch.bool), room_mask=torch.zeros(n, dtype=torch.bool))
            d.object_mask[extra:extra + n_obj] = True
            d.room_mask[2 * extra + n_obj:2 * extra + n_obj + n_room] = True
        out.append(d)
    return out


@pytest.mark.parametrize("data_type", ["homogeneous", "heterogeneous", "homogeneous_htree", "heterogeneous_htree"])
def test_restated_split_equals_the_masks_the_reference_wrote(data_type):
    z = np.load(GOLDEN)
    counts, extra = z["counts"].tolist(), int(z["htree_extra"])
    cases = sorted({k.split("/")[1] for k in z.files if k.startswith(data_type + "/")})
    assert cases == ["partial", "rest", "sum1"]
    for case in cases:
        ratios = [None if np.isnan(r) else float(r) for r in z[f"{data_type}/{case}/ratios"]]
        graphs = _fixture_graphs(data_type, counts, extra)
        nsr.generate_node_split(graphs, data_type, *ratios, seed=int(z[f"{data_type}/{case}/seed"]))
        keys = [k for k in z.files if k.startswith(f"{data_type}/{case}/") and k.endswith("_mask")]
        assert len(keys) == (6 if data_type.startswith("heterogeneous") else 3)
        for k in keys:
            t, m = k.split("/")[2:]
            got = torch.cat([getattr(g if t == "node" else g[t], m) for g in graphs]).numpy()
            assert got.dtype == np.bool_ and np.array_equal(got, z[k]), k
            assert z[k].any() or m != "train_mask"
        # the product's assignment vector against the same recorded masks: a homogeneous graph takes it in node order, the others
        # hand out as many of every kind
        assign = store.node_split_assignment(sum(a + b for a, b in counts), ratios, int(z[f"{data_type}/{case}/seed"]))
        for v, m in ((1, "train_mask"), (2, "val_mask"), (3, "test_mask")):
            recorded = [z[k] for k in keys if k.endswith("/" + m)]
            assert sum(int(r.sum()) for r in recorded) == int((assign == v).sum())
            if data_type == "homogeneous":
                assert np.array_equal(recorded[0], assign == v)


def test_store_dataset_quacks_like_the_reference_containers():
    class FakeStore:
        homogeneous, n_graphs, calls = False, 7, []

        def generate_node_split(self, *a, **k):
            self.calls.append((a, k))

    ds = store.StoreDataset(FakeStore(), "heterogeneous", {"objects": 9, "rooms": 6}, 15, 35)
    assert len(ds) == 7 and ds.data_type() == "heterogeneous"
    first = ds.get_data(0)
    assert first.num_node_features() == {"objects": 9, "rooms": 6} and first.num_room_labels() == 15 and first.num_object_labels() == 35
    ds.generate_node_split(0.7, 0.1, 0.2, seed=4)
    assert FakeStore.calls == [((0.7, 0.1, 0.2), {"seed": 4})]
    with pytest.raises(_lib.HydraMPError, match="no host graphs"):
        ds[0]
    with pytest.raises(_lib.HydraMPError, match="homogeneous"):
        store.StoreDataset(FakeStore(), "homogeneous", 6, 15)
    with pytest.raises(_lib.HydraMPError, match="unknown data type"):
        store.StoreDataset(FakeStore(), "typed", 6, 15)
