"""Device-collated batches of the two-headed (room + object) task: ``GraphStore`` keeps per-graph data with bool masks (and
homogeneous ``Data`` graphs), a two-headed ``BatchStream`` collates features, edges, labels and masks of both heads in ONE launch,
``semisupervised_step(...).run(stream.next(ids), mask=...)`` steps on it and ``count_correct`` / ``evaluate.semisupervised_accuracy``
count on it -- for HeterogeneousNetwork, HeterogeneousNeuralTreeNetwork, HomogeneousNetwork and HomogeneousNeuralTreeNetwork.

Every comparison is exact: the stream and the host path run the same kernels on the same bytes."""
import copy
import ctypes as C
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hydra_gnn_amd import _lib, evaluate, workloads  # noqa: E402
from hydra_gnn_amd.data import HeteroData, collate, collate_homogeneous  # noqa: E402
from hydra_gnn_amd.models import (HeterogeneousNetwork, HeterogeneousNeuralTreeNetwork, HomogeneousNetwork,  # noqa: E402
                                  HomogeneousNeuralTreeNetwork)
from hydra_gnn_amd.store import GraphStore  # noqa: E402

DEV = "cuda:0"
LR, WD = 0.002, 0.001
MASKS = ("train_mask", "val_mask", "test_mask")
GAT3 = dict(GAT_hidden_dims=[16, 16], GAT_heads=[2, 2, 2], GAT_concats=[True, True, False])
HT_DIMS = {"object": 306, "room": 6, "object-room": 6, "room-room": 6, "object_virtual": 306, "room_virtual": 6}

# the four data shapes of the task (graphs_of / model_of give each one's per-graph data and model)
SHAPES = ("hetero", "hetero_htree", "homog", "homog_htree")


def graphs_of(shape, n, seed, block="GraphSAGE"):
    edge = block == "GAT_edge"
    if shape == "hetero":
        return workloads.semisupervised_graphs(n, seed, relative_pos=edge)
    if shape == "hetero_htree":
        return workloads.semisupervised_htree_graphs(n, seed, relative_pos=edge)
    if shape == "homog":
        return workloads.stanford_semisupervised_graphs(n, seed, edge_attr=edge)
    return workloads.stanford_htree_semisupervised_graphs(n, seed, edge_attr=edge)


def model_of(shape, block="GraphSAGE", init=False, dropout=0.25):
    edge = block == "GAT_edge"
    if shape == "hetero":
        return HeterogeneousNetwork(input_dim_dict={"objects": 303 if edge else 306, "rooms": 3 if edge else 6},
                                    output_dim_dict={"rooms": 26, "objects": 28}, conv_block=block, hidden_dim=32, num_layers=3,
                                    dropout=dropout, **GAT3)
    if shape == "hetero_htree":
        return HeterogeneousNeuralTreeNetwork(input_dim_dict=dict(HT_DIMS),
                                              output_dim_dict={"room": 15, "object": 35, "object-room": 1, "room-room": 1},
                                              conv_block=block, hidden_dim=32, num_layers=3, disable_initialization=not init,
                                              dropout=dropout, **GAT3)
    kw = dict(input_dim=6, output_dim_dict={"room": 15, "object": 35}, conv_block=block, hidden_dim=32, num_layers=3, dropout=dropout)
    if block != "GraphSAGE":
        kw.update(GAT_hidden_dims=[16, 16], GAT_heads=[3, 3], GAT_concats=[True, True])
    if shape == "homog":
        return HomogeneousNetwork(**kw)
    return HomogeneousNeuralTreeNetwork(disable_initialization=not init, **kw)


def twin_nets(shape, block="GraphSAGE", init=False, seed=0):
    torch.manual_seed(seed)
    a = model_of(shape, block, init)
    if init and shape == "homog_htree":
        with torch.no_grad():
            a.pre_mp.bias.uniform_(-0.2, 0.2)
    b = copy.deepcopy(a)
    return a.to(DEV).train(), b.to(DEV).train()


def host_batch(shape, graphs, ids):
    sel = [graphs[i] for i in ids]
    return (collate_homogeneous(sel) if shape.startswith("homog") else collate(sel)).to(DEV)


def host_step(shape, net, step, gb, mask):
    """the step on a host-collated batch, through the interfaces that take data objects"""
    if shape.startswith("homog"):
        step(gb, None, getattr(gb, mask))
    else:
        types = net.native().head_label_types()
        step(gb, tuple(gb[t].y for t in types), None if mask is None else tuple(getattr(gb[t], mask) for t in types))


def host_count(shape, net, gb, mask, counts):
    if shape.startswith("homog"):
        return net.count_correct(gb, mask, counts)
    types = net.native().head_label_types()
    return net.count_correct(gb, tuple(gb[t].y for t in types), tuple(getattr(gb[t], mask) for t in types), counts)


def stream_count(shape, net, holder, mask, counts):
    if shape.startswith("homog"):
        return net.count_correct(holder, mask, counts)
    return net.count_correct(holder, None, mask, counts)


def inline_limit_batch(n_slots):
    """largest batch size whose tables (n_slots * (B + 1) + B int64 words) still travel in the kernel argument block (264 words)"""
    return (264 - n_slots) // (n_slots + 1)


# ---- 1. fails before, passes after ---------------------------------------------------------------------------------------------
def test_store_takes_bool_masks_and_the_two_head_step_runs_on_a_stream_batch():
    gs = workloads.semisupervised_graphs(10, seed=3)
    assert gs[0]["rooms"].train_mask.dtype == torch.bool
    store = GraphStore(gs, DEV)
    torch.manual_seed(0)
    net = model_of("hetero").to(DEV).train()
    stream = store.stream(net, 4)
    step = net.semisupervised_step(lr=LR, weight_decay=WD, use_graph=False)
    step.run(stream.next([1, 5, 2, 7]), mask="train_mask")
    assert np.isfinite(step.loss()) and net.native().read_state() == (1, 0)


# ---- 2. byte rows are bit-identical --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_bytes", [1, 2, 3, 5])
def test_collate_rows_of_odd_byte_sizes_equal_a_numpy_gather(row_bytes):
    lib = _lib.require_device()
    rng = np.random.default_rng(row_bytes)
    counts = rng.integers(0, 9, size=13)
    counts[4] = 0
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    src = rng.integers(0, 256, size=(int(ptr[-1]), row_bytes), dtype=np.uint8)
    sel = np.array([3, 4, 12, 3, 0, 7, 7], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(counts[sel])]).astype(np.int64)
    want = np.concatenate([src[ptr[g]:ptr[g + 1]] for g in sel], 0)
    d_src, d_ptr, d_sel, d_off = (torch.from_numpy(a).to(DEV) for a in (src, ptr, sel, off))
    guard = 16
    dst = torch.full((want.shape[0] * row_bytes + guard,), 0xAB, dtype=torch.uint8, device=DEV)
    _lib.check(lib.hmp_collate_rows(d_src.data_ptr(), row_bytes, d_ptr.data_ptr(), d_sel.data_ptr(), d_off.data_ptr(), len(sel),
                                    want.shape[0], dst.data_ptr(), _lib.stream_ptr()))
    got = dst.cpu().numpy()
    assert np.array_equal(got[:want.size].reshape(want.shape), want)
    assert (got[want.size:] == 0xAB).all()  # nothing written past the last row


@pytest.mark.parametrize("shape", SHAPES)
def test_store_collate_equals_host_collation_masks_included(shape):
    """GraphStore.collate (one gather per attribute): bool rows as they are; a store of homogeneous graphs returns a ``Data``"""
    gs = graphs_of(shape, 9, seed=12, block="GAT_edge")
    store = GraphStore(gs, DEV)
    for ids in ([4], [8, 0, 3, 3, 5], list(range(9))):
        got = store.collate(ids)
        if shape.startswith("homog"):
            ref = collate_homogeneous([gs[i] for i in ids])
            keys = [k for k, v in ref.__dict__.items() if isinstance(v, torch.Tensor)]
            assert [k for k, v in got.__dict__.items() if isinstance(v, torch.Tensor)] == keys and got.num_graphs == ref.num_graphs
            for k in keys:
                w, v = getattr(got, k), getattr(ref, k)
                assert w.is_cuda and w.dtype == v.dtype and torch.equal(w.cpu(), v), k
        else:
            ref = collate([gs[i] for i in ids])
            for t in ref.node_types:
                for k in ref[t].keys():
                    v = getattr(ref[t], k)
                    if isinstance(v, torch.Tensor):
                        w = getattr(got[t], k)
                        assert w.dtype == v.dtype and torch.equal(w.cpu(), v), (t, k)
            for e in ref.edge_types:
                assert torch.equal(got[e].edge_index.cpu(), ref[e].edge_index), e


def check_stream_batch(shape, stream, h, graphs, ids, it):
    got = stream.data()
    B = len(ids)
    sel = [graphs[i] for i in ids]
    carried = {(key, name) for _, key, name in stream._what}
    off = stream._offsets.view(-1, stream._off_stride).cpu()
    if shape.startswith("homog"):
        ref = collate_homogeneous(sel)
        from hydra_gnn_amd.store import HOMO_NODE, homo_edge_type

        n_checked = 0
        for k, v in ref.__dict__.items():
            if not isinstance(v, torch.Tensor):
                continue
            if "index" in k:
                e = homo_edge_type(k)
                if (e, "edge_index") in carried:
                    assert torch.equal(got[e].edge_index.cpu(), v), (it, k)
                    n_checked += 1
            elif k == "edge_attr":
                e = homo_edge_type("edge_index")
                if (e, k) in carried:
                    assert torch.equal(got[e].edge_attr.cpu(), v), (it, k)
                    n_checked += 1
            elif (HOMO_NODE, k) in carried:
                w = getattr(got[HOMO_NODE], k).cpu()
                assert w.dtype == v.dtype and torch.equal(w, v), (it, k)
                n_checked += 1
        assert n_checked == len(stream._what)
        ptr = torch.tensor(np.concatenate([[0], np.cumsum([g.num_nodes for g in sel])]))
        assert torch.equal(off[stream._slot_of[HOMO_NODE], :B + 1], ptr), it
        assert int(h.c.n_out) == ref.x.size(0)
    else:
        ref = collate(sel)
        for _, key, name in stream._what:
            w, v = getattr(got[key], name).cpu(), getattr(ref[key], name)
            assert w.dtype == v.dtype and torch.equal(w, v), (it, key, name)
        for key in stream._slots:
            assert torch.equal(off[stream._slot_of[key], :B + 1], ref[key].ptr), (it, key)
    assert int(h.c.n_graphs) == B


@pytest.mark.parametrize("side", ["inline", "ring"])
@pytest.mark.parametrize("shape", SHAPES)
def test_two_headed_stream_is_bit_identical_to_host_collation(shape, side):
    block = "GAT_edge" if shape in ("hetero_htree", "homog") else "GraphSAGE"  # edge_attr rides along in two of the shapes
    n_graphs = 30
    gs = graphs_of(shape, n_graphs, seed=17, block=block)
    if shape == "hetero":  # a graph in which one head's node type is empty: rooms without objects
        g = gs[3]
        e = HeteroData()
        e["objects"].x = g["objects"].x[:0]
        e["objects"].pos = g["objects"].pos[:0]
        e["objects"].y = g["objects"].y[:0]
        e["rooms"].x, e["rooms"].pos, e["rooms"].y = g["rooms"].x, g["rooms"].pos, g["rooms"].y
        for t in ("objects", "rooms"):
            for m in MASKS:
                setattr(e[t], m, getattr(g[t], m)[: int(e[t].y.numel())])
        for et in g.edge_types:
            e[et].edge_index = g[et].edge_index if et[0] == et[2] == "rooms" else torch.empty((2, 0), dtype=torch.int64)
        gs[3] = e
    store = GraphStore(gs, DEV)
    torch.manual_seed(0)
    net = model_of(shape, block).to(DEV)
    probe = store.stream(net, 1)
    limit = inline_limit_batch(len(probe._slots))
    assert limit >= 2
    batch_size = limit if side == "inline" else limit + 1
    stream = store.stream(net, batch_size)
    names = {name for _, _, name in stream._what}
    assert set(MASKS) <= names and "y" in names and "pos" not in names  # targets ride along, unread attributes do not
    rng = np.random.default_rng(1)
    saw_odd = False
    for it in range(13):  # > the ring depth of 8
        B = batch_size if it % 3 else max(batch_size // 2, 1)  # short batches too
        ids = rng.choice(n_graphs, size=B, replace=True).tolist()
        if it == 2 and shape == "hetero":
            ids[0] = 3
        h = stream.next(ids)
        check_stream_batch(shape, stream, h, gs, ids, it)
        saw_odd = saw_odd or any(int(v) % 4 for v in stream._totals)
    assert saw_odd  # node totals that are not multiples of 4 were among them


# ---- 3. the step is the host step ----------------------------------------------------------------------------------------------
STEP_CASES = [("hetero", "GraphSAGE", False, "train_mask"), ("hetero", "GAT_edge", False, "train_mask"),
              ("hetero", "GraphSAGE", False, None), ("hetero_htree", "GraphSAGE", False, "train_mask"),
              ("homog", "GraphSAGE", False, "train_mask"), ("homog_htree", "GraphSAGE", False, "train_mask"),
              ("homog_htree", "GraphSAGE", True, "train_mask")]


@pytest.mark.parametrize("shape,block,init,mask", STEP_CASES)
def test_stream_step_is_the_host_step(shape, block, init, mask):
    n_graphs = 40
    gs = graphs_of(shape, n_graphs, seed=4, block=block)
    store = GraphStore(gs, DEV)
    net_a, net_b = twin_nets(shape, block, init)
    step_a = net_a.semisupervised_step(lr=LR, weight_decay=WD, use_graph=False)
    step_b = net_b.semisupervised_step(lr=LR, weight_decay=WD, use_graph=False)
    stream = store.stream(net_a, 8)
    rng = np.random.default_rng(2)
    for it in range(10):
        ids = rng.choice(n_graphs, size=8 if it != 6 else 5, replace=False).tolist()
        step_a.run(stream.next(ids), mask=mask)
        host_step(shape, net_b, step_b, host_batch(shape, gs, ids), mask)
        la, lb = step_a.loss(), step_b.loss()
        print(f"{shape} {block} init={init} mask={mask} step {it}: stream loss {la!r}, host loss {lb!r}")
        assert la == lb, it
    for (n, p), (_, q) in zip(net_a.named_parameters(), net_b.named_parameters()):
        assert torch.equal(p, q), n
    assert net_a.native().read_state() == (10, 0)


# ---- 4. counting is the host count ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_stream_count_is_the_host_count_and_accuracy_is_the_reference_formula(shape):
    n_graphs = 24
    gs = graphs_of(shape, n_graphs, seed=9)
    store = GraphStore(gs, DEV)
    torch.manual_seed(1)
    net = model_of(shape).to(DEV)
    stream = store.stream(net, 7)
    id_lists = [list(range(i, min(i + 7, n_graphs))) for i in range(0, n_graphs, 7)]
    for mask in MASKS:
        c_stream = torch.zeros(4, dtype=torch.int64, device=DEV)
        c_host = torch.zeros(4, dtype=torch.int64, device=DEV)
        for ids in id_lists:
            assert stream_count(shape, net, stream.next(ids), mask, c_stream) is c_stream
            host_count(shape, net, host_batch(shape, gs, ids), mask, c_host)
        a, b = c_stream.tolist(), c_host.tolist()
        print(f"{shape} {mask}: stream {a}, host {b}")
        assert a == b and a[1] > 0 and a[3] > 0
        cr, tr, co, to = b
        acc = evaluate.semisupervised_accuracy(net, (stream, id_lists), mask)
        assert acc == (cr + co) / (tr + to)
        assert evaluate.semisupervised_accuracy(net, (stream, id_lists), mask, type_separated=True) == (cr / tr, co / to)
        assert evaluate.semisupervised_accuracy(net, [host_batch(shape, gs, ids) for ids in id_lists], mask) == acc


# ---- 5. one launch -------------------------------------------------------------------------------------------------------------
def step_launches(net, fn):
    fn()  # warm (workspace, handle)
    torch.cuda.synchronize()
    h, lib = net.native()._handle, net.native()._lib
    _lib.check(lib.hmp_net_profile(h, 1))
    fn()
    torch.cuda.synchronize()
    ms = np.zeros(_lib.N_KCLASS, dtype=np.float32)
    n = np.zeros(_lib.N_KCLASS, dtype=np.int32)
    _lib.check(lib.hmp_net_profile_read(h, ms.ctypes.data_as(C.POINTER(C.c_float)), n.ctypes.data_as(C.POINTER(C.c_int32))))
    _lib.check(lib.hmp_net_profile(h, 0))
    return n.tolist()


@pytest.mark.parametrize("shape,block", [("hetero", "GraphSAGE"), ("hetero_htree", "GAT_edge"), ("homog", "GraphSAGE"),
                                         ("homog_htree", "GraphSAGE")])
def test_run_enqueues_the_launches_of_the_host_batch_step(shape, block):
    """launch counts per kernel class (hmp_net_profile_read) of run(stream batch) and of step(host batch) on the same graphs; the
    H-tree GAT_edge shape (21 slots, 39 items with every mask) must fit ONE collator call"""
    gs = graphs_of(shape, 16, seed=6, block=block)
    store = GraphStore(gs, DEV)
    net_a, net_b = twin_nets(shape, block, init=shape == "hetero_htree")  # with pre_mp the net reads all 15 edge types
    step_a = net_a.semisupervised_step(lr=LR, weight_decay=WD, use_graph=False)
    step_b = net_b.semisupervised_step(lr=LR, weight_decay=WD, use_graph=False)
    stream = store.stream(net_a, 8)
    if shape == "hetero_htree":
        assert len(stream._slots) == 21 and len(stream._what) == 39
    ids = [3, 0, 9, 9, 14, 1, 7, 5]
    holder = stream.next(ids)
    gb = host_batch(shape, gs, ids)
    n_stream = step_launches(net_a, lambda: step_a.run(holder, mask="train_mask"))
    n_host = step_launches(net_b, lambda: host_step(shape, net_b, step_b, gb, "train_mask"))
    print(f"{shape} {block}: launches per class, stream {n_stream} (sum {sum(n_stream)}), host {n_host} (sum {sum(n_host)})")
    assert n_stream == n_host


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_attribute_and_leave_the_net_usable():
    gs = workloads.semisupervised_graphs(8, seed=5)
    torch.manual_seed(0)
    net = model_of("hetero").to(DEV).train()
    step = net.semisupervised_step(lr=LR, weight_decay=WD, use_graph=False)

    def variant(edit):
        out = copy.deepcopy(gs)
        for g in out:
            edit(g)
        return GraphStore(out, DEV)

    with pytest.raises(_lib.HydraMPError, match="val_mask"):  # a needed attribute is missing
        variant(lambda g: delattr(g["objects"], "val_mask")).stream(net, 4)
    with pytest.raises(_lib.HydraMPError, match="'y'.*int64"):  # labels that are not int64
        variant(lambda g: setattr(g["rooms"], "y", g["rooms"].y.to(torch.int32))).stream(net, 4)
    with pytest.raises(_lib.HydraMPError, match="'test_mask'.*bool"):  # masks that are not bool
        variant(lambda g: setattr(g["rooms"], "test_mask", g["rooms"].test_mask.to(torch.uint8))).stream(net, 4)
    store = GraphStore(gs, DEV)
    with pytest.raises(_lib.HydraMPError, match="label_type"):
        store.stream(net, 4, "rooms")
    bare = store.stream(net, 4, targets=False)
    with pytest.raises(_lib.HydraMPError, match="no targets"):
        step.run(bare.next([0, 1]))
    stream = store.stream(net, 4, masks=("train_mask",))
    with pytest.raises(_lib.HydraMPError, match="val_mask"):
        step.run(stream.next([0, 1]), mask="val_mask")
    from hydra_gnn_amd.engine import TrainStep

    single = TrainStep(net.native(), lr=LR, use_graph=False)
    with pytest.raises(_lib.HydraMPError, match="two-headed stream"):
        single.run(stream.next([0, 1]))
    graphed = net.semisupervised_step(lr=LR, weight_decay=WD)
    with pytest.raises(_lib.HydraMPError, match="use_graph=False"):
        graphed.run(stream.next([0, 1]))
    torch.manual_seed(0)
    other = model_of("hetero").to(DEV).train()
    with pytest.raises(_lib.HydraMPError, match="another model"):
        other.semisupervised_step(lr=LR, use_graph=False).run(stream.next([0, 1]))
    # the net is still usable
    step.run(stream.next([2, 3, 4]), mask="train_mask")
    assert np.isfinite(step.loss()) and net.native().read_state() == (1, 0)
    # a label outside the head's classes sets status bit 2 through the step, as with host batches
    bad = variant(lambda g: g["rooms"].y.fill_(26))
    torch.manual_seed(0)
    net2 = model_of("hetero").to(DEV).train()
    step2 = net2.semisupervised_step(lr=LR, weight_decay=WD, use_graph=False)
    step2.run(bad.stream(net2, 4).next([0, 1]), mask=None)
    assert net2.native().read_state()[1] & 2


# ---- the time ------------------------------------------------------------------------------------------------------------------
def test_stream_epoch_beats_host_collation_epoch():
    """one epoch of 20 shuffled batches of 16 Stanford-like graphs: host collate + H2D + step(batch) against stream + run"""
    n_graphs, bs = 320, 16
    gs = workloads.stanford_semisupervised_graphs(n_graphs, seed=31)
    store = GraphStore(gs, DEV)
    net_a, net_b = twin_nets("homog")
    step_a = net_a.semisupervised_step(lr=LR, weight_decay=WD, use_graph=False)
    step_b = net_b.semisupervised_step(lr=LR, weight_decay=WD, use_graph=False)
    stream = store.stream(net_a, bs)
    rng = np.random.default_rng(0)

    def epoch(stream_mode):
        perm = rng.permutation(n_graphs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(0, n_graphs, bs):
            ids = perm[i:i + bs]
            if stream_mode:
                step_a.run(stream.next(ids), mask="train_mask")
            else:
                step_b(collate_homogeneous([gs[j] for j in ids]).to(DEV))
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    epoch(True), epoch(False)  # warm-up
    t_stream = min(epoch(True) for _ in range(5))
    t_host = min(epoch(False) for _ in range(5))
    print(f"semi-supervised epoch, {n_graphs} graphs in batches of {bs}: stream {1e3 * t_stream:.2f} ms, host {1e3 * t_host:.2f} ms")
    assert t_stream < t_host
