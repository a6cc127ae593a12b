"""``GraphStore.generate_node_split`` on the device (``hmp_store_node_split``, one wave per graph) against the reference's
``Stanford3DSG_dataset.generate_node_split`` restated over host copies of the graphs (``tests/_node_split_reference.py``, pinned to the
reference's own masks by ``tests/test_store_derive_host.py``), on all four data types.  Bit-exact.  The mask rows are allocated
pre-filled with 0xA5, so a row the launch never writes cannot pass by luck."""
import numpy as np
import pytest
import torch

import _node_split_reference as nsr
import _store_derive_cases as sc
from hydra_gnn_amd import store as hstore
from hydra_gnn_amd.data import collate
from hydra_gnn_amd.models import HeterogeneousNetwork
from hydra_gnn_amd.store import DEFAULT_MASKS, HOMO_NODE, GraphStore

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DATA_TYPES = ["heterogeneous", "heterogeneous_htree", "homogeneous", "homogeneous_htree"]
COUNTS6 = sc.BASELINE_COUNTS + [(2, 2)]
PARTS = {"heterogeneous": ["objects", "rooms"], "heterogeneous_htree": ["object_virtual", "room_virtual"], "homogeneous": [HOMO_NODE],
         "homogeneous_htree": [HOMO_NODE]}
_HOST = {}


@pytest.fixture(autouse=True)
def prefilled_outputs(monkeypatch):
    def alloc(shape, dtype, device):
        t = torch.empty(shape, dtype=dtype, device=device)
        if t.numel():
            t.reshape(-1).view(torch.uint8).fill_(0xA5)
        return t

    monkeypatch.setattr(hstore, "_derive_alloc", alloc)


def host_graphs(data_type):
    """6 host graphs of a data type (never modified: every user clones)"""
    if data_type not in _HOST:
        typed = sc.htree_graphs(True, n=6) if data_type.endswith("htree") else sc.baseline_graphs(True, counts=COUNTS6, ro_edges=True)
        _HOST[data_type] = typed if data_type.startswith("heterogeneous") else [sc.homogeneous(sc.clone(g)) for g in typed]
    return _HOST[data_type]


def resident(data_type):
    """the store of a data type; the homogeneous ones are derived on the device from the typed store"""
    if data_type.startswith("heterogeneous"):
        return GraphStore(host_graphs(data_type), DEV)
    return GraphStore(host_graphs("heterogeneous" + data_type[len("homogeneous"):]), DEV).to_homogeneous()


def oracle(data_type, ratios, seed):
    graphs = [sc.clone(g) for g in host_graphs(data_type)]
    nsr.generate_node_split(graphs, data_type, *ratios, seed=seed)
    return GraphStore(graphs, DEV)


def masks_of(store, data_type):
    return {(t, k): store.node_attrs[t][k].data for t in PARTS[data_type] for k in DEFAULT_MASKS}


@pytest.mark.parametrize("ratios", [(0.7, 0.1, 0.2), (0.4, 0.2, 0.2), (0.5, 0.2, None)])
@pytest.mark.parametrize("data_type", DATA_TYPES)
def test_masks_equal_the_restated_reference(data_type, ratios):
    store = resident(data_type)
    store.generate_node_split(*ratios, seed=1)
    torch.cuda.synchronize()
    sc.assert_same_store(store, oracle(data_type, ratios, 1))
    # disjoint, and as many as the rounded targets
    m = masks_of(store, data_type)
    stack = {k: torch.cat([m[(t, k)] for t in PARTS[data_type]]).view(torch.uint8) for k in DEFAULT_MASKS}
    assert int((stack["train_mask"] + stack["val_mask"] + stack["test_mask"]).max()) == 1
    total = sum(nsr.num_graph_nodes(g, data_type) for g in host_graphs(data_type))
    test = 1 - ratios[0] - ratios[1] if ratios[2] is None else ratios[2]
    n_train, n_val = round(total * ratios[0]), round(total * ratios[1])
    n_test = total - n_train - n_val if ratios[0] + ratios[1] + test == 1 else round(total * test)
    assert [int(stack[k].sum()) for k in DEFAULT_MASKS] == [n_train, n_val, n_test]
    if data_type == "homogeneous_htree":  # only the virtual rows are ever assigned
        member = store.node_attrs[HOMO_NODE]["room_mask"].data | store.node_attrs[HOMO_NODE]["object_mask"].data
        assert not bool(((stack["train_mask"] + stack["val_mask"] + stack["test_mask"]).bool() & ~member).any())


@pytest.mark.parametrize("data_type", DATA_TYPES)
def test_a_second_seed_differs_and_the_first_comes_back_in_the_same_tensors(data_type):
    ratios = (0.7, 0.1, 0.2)
    store = resident(data_type)
    store.generate_node_split(*ratios, seed=0)
    ptrs = {k: v.data_ptr() for k, v in masks_of(store, data_type).items()}
    first = {k: v.clone() for k, v in masks_of(store, data_type).items()}
    store.generate_node_split(*ratios, seed=5)
    second = {k: v.clone() for k, v in masks_of(store, data_type).items()}
    assert any(not torch.equal(first[k], second[k]) for k in first)
    sc.assert_same_store(store, oracle(data_type, ratios, 5))
    store.generate_node_split(*ratios, seed=0)
    assert {k: v.data_ptr() for k, v in masks_of(store, data_type).items()} == ptrs
    for k, v in masks_of(store, data_type).items():
        assert torch.equal(v.view(torch.uint8), first[k].view(torch.uint8)), k
    sc.assert_same_store(store, oracle(data_type, ratios, 0))


def test_an_open_stream_carries_the_new_split_at_its_next_batch():
    ratios = (0.7, 0.1, 0.2)
    store = resident("heterogeneous")
    store.generate_node_split(*ratios, seed=0)
    torch.manual_seed(0)
    net = HeterogeneousNetwork(input_dim_dict={"objects": sc.OBJ_W, "rooms": sc.ROOM_W}, output_dim_dict={"rooms": 15, "objects": 15},
                               conv_block="GraphSAGE", hidden_dim=16, num_layers=2).to(DEV)
    stream = store.stream(net, 3)
    ids = [5, 0, 3]
    for it, seed in enumerate((0, 5, 0)):
        if it:  # the stream stays open: no new stream, no new buffers
            store.generate_node_split(*ratios, seed=seed)
        stream.next(ids)
        got = stream.data()
        want = collate([sc.clone(g) for g in _with_split("heterogeneous", ratios, seed, ids)]).to(DEV)
        for t in ("objects", "rooms"):
            for k in DEFAULT_MASKS:
                assert torch.equal(getattr(got[t], k), getattr(want[t], k)), (seed, t, k)


def _with_split(data_type, ratios, seed, ids):
    graphs = [sc.clone(g) for g in host_graphs(data_type)]
    nsr.generate_node_split(graphs, data_type, *ratios, seed=seed)
    return [graphs[i] for i in ids]


def test_derived_stores_split_apart_from_their_parent():
    parent = resident("heterogeneous")
    parent.generate_node_split(0.7, 0.1, 0.2, seed=0)
    child = parent.with_relative_pos()
    before = {k: v.clone() for k, v in masks_of(parent, "heterogeneous").items()}
    child.generate_node_split(0.7, 0.1, 0.2, seed=5)
    for k, v in masks_of(parent, "heterogeneous").items():
        assert torch.equal(v, before[k]) and v.data_ptr() != masks_of(child, "heterogeneous")[k].data_ptr()
    want = oracle("heterogeneous", (0.7, 0.1, 0.2), 5)
    for k, v in masks_of(child, "heterogeneous").items():
        assert torch.equal(v.view(torch.uint8), masks_of(want, "heterogeneous")[k].view(torch.uint8)), k


def test_member_counts_are_read_once(monkeypatch):
    store = resident("homogeneous_htree")
    reads = []
    cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (reads.append(tuple(self.shape)), cpu(self, *a, **k))[1])
    store.generate_node_split(0.7, 0.1, 0.2, seed=0)
    assert reads == [(2, 6)]
    store.generate_node_split(0.7, 0.1, 0.2, seed=1)
    assert reads == [(2, 6)]
    typed = resident("heterogeneous")
    typed.generate_node_split(0.7, 0.1, 0.2, seed=0)
    assert reads == [(2, 6)]
