"""Device-collated batches of the room task on homogeneous graphs: ``store.stream(model, B, label_type="node")`` for a
``HomogeneousNetwork`` / ``HomogeneousNeuralTreeNetwork`` built with ``output_dim`` collates ``x``, the edge lists, ``edge_attr``,
``room_mask`` and the room-masked labels (``room_mask ? y : ignored_label``, written by the collation launch:
``hmp_collator_set_label_filter``) in ONE launch; ``train_step(...).run`` steps on it, ``count_correct_rooms`` counts on it.

Every comparison is exact: the stream and ``store.collate`` run the same kernels on the same bytes.

The H-tree graphs are the ones ``tests/test_gpu_training_job.py`` builds from the topology fixture (306-d features); the model with
``pre_mp`` reads their first 6 columns, because ``pre_mp`` holds at most 256 channels."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hydra_gnn_amd import _lib, evaluate, workloads  # noqa: E402
from hydra_gnn_amd.data import heterogeneous_htree_to_homogeneous  # noqa: E402
from hydra_gnn_amd.models import HomogeneousNetwork, HomogeneousNeuralTreeNetwork  # noqa: E402
from hydra_gnn_amd.store import HOMO_NODE, GraphStore, homo_edge_type  # noqa: E402

DEV = "cuda:0"
LR, WD = 0.004, 0.001
IGNORED = 25
N_GRAPHS = 12
CASES = ("sage", "gat_edge", "htree_sage", "htree_gat_init")
GAT = dict(GAT_hidden_dims=[16], GAT_heads=[2, 2], GAT_concats=[True, False])


def stanford_graphs(n, seed, edge_attr=False):
    rng = np.random.default_rng(seed)
    gs = [workloads.stanford_like_graph(rng) for _ in range(n)]
    gs[3].y[0] = IGNORED  # a graph whose only room carries the ignored label: every row of it is filtered
    if edge_attr:
        for g in gs:
            g.edge_attr = (g.x[g.edge_index[1], :3] - g.x[g.edge_index[0], :3]).contiguous()
    return gs


def homog_htree_graphs(n, seed, feature_dim=None):
    """tests/test_gpu_training_job.py::_homog_htree_graphs; ``feature_dim``: keep the first columns of ``x``"""
    npz = np.load(workloads.HTREE_FIXTURE)
    rng = np.random.Generator(np.random.PCG64(seed))
    k = int(npz["n_graphs"])
    out = []
    for i in range(n):
        d = heterogeneous_htree_to_homogeneous(workloads.htree_graph(npz, i % k, rng))
        del d.__dict__["edge_type"]
        if feature_dim is not None:
            d.x = d.x[:, :feature_dim].contiguous()
        out.append(d)
    out[3].y[out[3].room_mask] = IGNORED
    return out


def case_of(name, dropout=0.25):
    """(graphs, model) of a case, the model seeded"""
    torch.manual_seed(5)
    if name == "sage":
        return stanford_graphs(N_GRAPHS, 1), HomogeneousNetwork(input_dim=6, output_dim=15, conv_block="GraphSAGE", hidden_dim=16,
                                                               num_layers=2, dropout=dropout)
    if name == "gat_edge":
        return stanford_graphs(N_GRAPHS, 2, edge_attr=True), HomogeneousNetwork(input_dim=6, output_dim=15, conv_block="GAT_edge",
                                                                                dropout=dropout, **GAT)
    if name == "htree_sage":
        return homog_htree_graphs(N_GRAPHS, 3), HomogeneousNeuralTreeNetwork(input_dim=306, output_dim=26, conv_block="GraphSAGE",
                                                                             hidden_dim=16, num_layers=2, dropout=dropout,
                                                                             disable_initialization=True)
    assert name == "htree_gat_init"
    net = HomogeneousNeuralTreeNetwork(input_dim=6, output_dim=26, conv_block="GAT", dropout=dropout, **GAT)
    with torch.no_grad():
        net.pre_mp.bias.uniform_(-0.2, 0.2)
    return homog_htree_graphs(N_GRAPHS, 4, feature_dim=6), net


def where_labels(b):
    return torch.where(b.room_mask, b.y, torch.full_like(b.y, IGNORED))


def check_batch(stream, h, store, ids, net):
    ref = store.collate(ids)
    got = stream.data()
    assert got.num_graphs == len(ids) and int(h.c.n_graphs) == len(ids) and int(h.c.n_out) == ref.x.size(0)
    assert torch.equal(got[HOMO_NODE].x, ref.x)
    assert torch.equal(got[HOMO_NODE].room_mask, ref.room_mask) and got[HOMO_NODE].room_mask.dtype == torch.bool
    names = ["edge_index", "pool_edge_index"] if isinstance(net, HomogeneousNeuralTreeNetwork) else ["edge_index"]
    if getattr(net, "pre_mp", None) is not None:
        names.append("init_edge_index")
    for k in names:
        assert torch.equal(got[homo_edge_type(k)].edge_index, getattr(ref, k)), k
    if net.conv_block == "GAT_edge":
        assert torch.equal(got[homo_edge_type("edge_index")].edge_attr, ref.edge_attr)
    want = where_labels(ref)
    n = ref.x.size(0)
    assert stream.label_buf.data_ptr() == h.c.d_labels and torch.equal(stream.label_buf[:n], want)
    assert torch.equal(got[HOMO_NODE].y, want)
    assert torch.equal(stream.members[:n], ref.room_mask)
    # nothing else the store holds
    assert len(stream._what) == 3 + len(names) + (net.conv_block == "GAT_edge")
    return ref, want


# ---- 1. collation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_stream_batches_equal_store_collate_with_room_masked_labels(name):
    gs, net = case_of(name)
    net = net.to(DEV)
    store = GraphStore(gs, DEV)
    stream = store.stream(net, 4, label_type="node", ignored_label=IGNORED)
    for ids in ([0, 1, 2, 5], [7], [4, 4, 9, 4], [3, 3], [2, 3, 6]):
        h = stream.next(ids)
        ref, want = check_batch(stream, h, store, ids, net)
        if ids == [3, 3]:
            assert bool((want == IGNORED).all())  # all rows filtered
        else:
            assert int((want != IGNORED).sum()) > 0
    # 96 graphs drawn from 12: the offset tables no longer fit the kernel's argument block and travel through the pinned ring
    big = store.stream(net, 96, label_type="node", ignored_label=IGNORED)
    rng = np.random.default_rng(9)
    for _ in range(2):
        ids = rng.integers(0, N_GRAPHS, size=96).tolist()
        n_slots = len(big._slots)
        assert n_slots * (len(ids) + 1) + len(ids) > 264
        check_batch(big, big.next(ids), store, ids, net)
    check_batch(big, big.next([1, 8]), store, [1, 8], net)  # and back to inline tables on the same collator


# ---- 2. the step ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_step_on_stream_batches_is_bit_equal_to_the_step_on_collated_batches(name):
    gs, a = case_of(name)
    b = copy.deepcopy(a)
    a, b = a.to(DEV).train(), b.to(DEV).train()
    store = GraphStore(gs, DEV)
    stream = store.stream(a, 4, label_type="node", ignored_label=IGNORED)
    sa = a.train_step(lr=LR, weight_decay=WD, ignored_label=IGNORED, use_graph=False)
    sb = b.train_step(lr=LR, weight_decay=WD, ignored_label=IGNORED, use_graph=False)
    for it, ids in enumerate(([0, 1, 2, 5], [4, 4, 9, 3], [7], [11, 10, 6, 8])):
        sa.run(stream.next(ids))
        gb = store.collate(ids)
        sb(gb, where_labels(gb))
        la, lb = sa.loss(), sb.loss()
        print(name, "step", it, "loss", la, lb)
        assert la == lb and np.isfinite(la), it
        assert torch.equal(sa.flat, sb.flat), it
        assert torch.equal(sa.m, sb.m) and torch.equal(sa.v, sb.v), it
    assert a.native().read_state() == (4, 0) and b.native().read_state() == (4, 0)


# ---- 3. counts ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_counts_on_stream_batches_equal_counts_on_collated_batches(name):
    gs, net = case_of(name)
    net = net.to(DEV).eval()
    C = net.native().n_classes
    store = GraphStore(gs, DEV)
    stream = store.stream(net, 6, label_type="node", ignored_label=IGNORED)
    got, want = torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV)
    got_m, want_m = torch.zeros(C, C, dtype=torch.int64, device=DEV), torch.zeros(C, C, dtype=torch.int64, device=DEV)
    batches = ([0, 1, 2, 3, 4, 5], [6, 7, 8, 9, 10])
    for ids in batches:
        net.count_correct_rooms(stream.next(ids), got, got_m, IGNORED)
        net.count_correct_rooms(store.collate(ids), want, want_m, IGNORED)
    print(name, "counts", got.tolist(), want.tolist())
    assert got.tolist() == want.tolist() and got[1] > 0
    assert torch.equal(got_m, want_m) and int(got_m.sum()) == int(got[1])
    acc = evaluate.accuracy(net, (stream, batches), IGNORED)
    assert acc == int(want[0]) / int(want[1])
    assert net.count_correct_rooms(stream.next(batches[1])) == net.count_correct_rooms(store.collate(batches[1]))


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals():
    gs, net = case_of("sage")
    net = net.to(DEV)
    E = _lib.HydraMPError
    bare = copy.deepcopy(gs)
    for g in bare:
        del g.__dict__["room_mask"]
    with pytest.raises(E, match="room_mask"):
        GraphStore(bare, DEV).stream(net, 4, label_type="node")
    bytes_ = copy.deepcopy(gs)
    for g in bytes_:
        g.room_mask = g.room_mask.to(torch.uint8)
    with pytest.raises(E, match="room_mask"):
        GraphStore(bytes_, DEV).stream(net, 4, label_type="node")
    narrow = copy.deepcopy(gs)
    for g in narrow:
        g.y = g.y.to(torch.int32)
    with pytest.raises(E, match="'y'"):
        GraphStore(narrow, DEV).stream(net, 4, label_type="node")
    store = GraphStore(gs, DEV)
    with pytest.raises(E, match="label_type"):
        store.stream(net, 4)
    torch.manual_seed(0)
    two = HomogeneousNetwork(input_dim=6, output_dim_dict={"room": 15, "object": 35}, conv_block="GraphSAGE", hidden_dim=16,
                             num_layers=2).to(DEV)
    with pytest.raises(E, match="two-headed"):
        store.stream(two, 4, label_type="node")
    stream = store.stream(net, 4, label_type="node", ignored_label=IGNORED)
    h = stream.next([0, 1])
    with pytest.raises(E, match="ignored_label"):
        net.train_step(lr=LR, ignored_label=IGNORED - 1, use_graph=False).run(h)
    counts = torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(E, match="ignored_label"):
        net.count_correct_rooms(h, counts, None, IGNORED - 1)
    assert counts.tolist() == [0, 0]  # nothing was counted on the wrong rows
    with pytest.raises(E, match="use_graph"):
        net.train_step(lr=LR, ignored_label=IGNORED, use_graph=True).run(h)
    gcn = HomogeneousNetwork(input_dim=6, output_dim=15, conv_block="GCN", hidden_dim=16, num_layers=2).to(DEV)
    with pytest.raises(E):
        store.stream(gcn, 4, label_type="node")
