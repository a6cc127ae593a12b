"""Predicted labels through the executor: model.predict / model.predict_labels on all four model classes and both tasks, on host
batches and on store.BatchStream descriptors, evaluate.predict and the jobs' predict().

What is compared with what.  The heterogeneous two-headed nets predict from the z and the activation forward() uses: predict()
equals the first-maximum argmax of the eval-mode model(batch) outputs exactly.  The homogeneous two-headed nets compute their
heads' logits on the VALU where forward() uses the MFMA GEMM, so a row (and head) is compared unless the float64 top-two gap of
the oracle's logits (oracle/models.py, same weights) is at most 64 x the largest |float32 oracle - float64 oracle| logit of the batch
-- at most 1 % of the rows, asserted on the CPU before the model runs.  Stream batches and store.collate batches run the same kernels
on the same bytes: bit-equal."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _tail_reference import _first_argmax, _top2_gap  # noqa: E402
from hydra_gnn_amd import _lib, evaluate, jobs, workloads  # noqa: E402
from hydra_gnn_amd.data import collate, collate_homogeneous, heterogeneous_htree_to_homogeneous  # noqa: E402
from hydra_gnn_amd.models import (HeterogeneousNetwork, HeterogeneousNeuralTreeNetwork, HomogeneousNetwork,  # noqa: E402
                                  HomogeneousNeuralTreeNetwork)
from hydra_gnn_amd.store import GraphStore  # noqa: E402
from oracle import models as omodels  # noqa: E402

DEV = "cuda:0"
KC_LOSS = 4  # kernel class of the loss / count / label launches (hmp_net_profile_read)
GAT3 = dict(GAT_hidden_dims=[16, 16], GAT_heads=[2, 2, 2], GAT_concats=[True, True, False])
GAT2 = dict(GAT_hidden_dims=[16, 16], GAT_heads=[3, 3], GAT_concats=[True, True])
HT_DIMS = {"object": 306, "room": 6, "object-room": 6, "room-room": 6, "object_virtual": 306, "room_virtual": 6}
SHAPES = ("hetero", "hetero_htree", "homog", "homog_htree")


def graphs_of(shape, n, seed):
    return {"hetero": workloads.semisupervised_graphs, "hetero_htree": workloads.semisupervised_htree_graphs,
            "homog": workloads.stanford_semisupervised_graphs, "homog_htree": workloads.stanford_htree_semisupervised_graphs}[shape](n, seed)


def two_head_kw(shape, block):
    if shape == "hetero":
        return dict(input_dim_dict={"objects": 306, "rooms": 6}, output_dim_dict={"rooms": 26, "objects": 28}, conv_block=block,
                    hidden_dim=32, num_layers=3, **GAT3)
    if shape == "hetero_htree":
        return dict(input_dim_dict=dict(HT_DIMS), output_dim_dict={"room": 15, "object": 35, "object-room": 1, "room-room": 1},
                    conv_block=block, hidden_dim=32, num_layers=3, disable_initialization=True, **GAT3)
    kw = dict(input_dim=6, output_dim_dict={"room": 15, "object": 35}, conv_block=block, hidden_dim=32, num_layers=3)
    if block != "GraphSAGE":
        kw.update(GAT2)
    if shape == "homog_htree":
        kw["disable_initialization"] = True
    return kw


CLASS_OF = {"hetero": HeterogeneousNetwork, "hetero_htree": HeterogeneousNeuralTreeNetwork, "homog": HomogeneousNetwork,
            "homog_htree": HomogeneousNeuralTreeNetwork}


def two_head_model(shape, block="GraphSAGE", seed=0):
    torch.manual_seed(seed)
    net = CLASS_OF[shape](**two_head_kw(shape, block))
    with torch.no_grad():  # biases away from 0, so that ReLU rows of zeros are not the rule
        for name, p in net.named_parameters():
            if name.endswith("bias"):
                p.add_(torch.randn_like(p) * 0.2)
    return net


def host_batch(shape, graphs, ids):
    sel = [graphs[i] for i in ids]
    return (collate_homogeneous(sel) if shape.startswith("homog") else collate(sel)).to(DEV)


def eval_outputs(net, batch):
    net.eval()
    with torch.no_grad():
        out = net(batch)
    return [o.cpu() for o in (out if isinstance(out, tuple) else (out,))]


def oracle_compared_rows(shape, block, net, batch):
    """per head: the rows the gap rule compares, from the oracle alone (float64 logits, the float32 oracle as yardstick)"""
    kw = two_head_kw(shape, block)
    ora = (omodels.HomogeneousNeuralTreeNetwork if shape == "homog_htree" else omodels.HomogeneousNetwork)(**kw)
    ora.load_state_dict({k: v.detach().cpu() for k, v in net.state_dict().items()}, strict=True)
    ora.eval()
    b32 = batch.to("cpu")
    b64 = batch.to("cpu")
    b64.x = b64.x.double()
    with torch.no_grad():
        l32 = ora(b32)
        l64 = copy.deepcopy(ora).double()(b64)
    bound = 64.0 * max(float((a.double() - b).abs().max()) for a, b in zip(l32, l64))
    use = []
    for h, l in enumerate(l64):
        skip = _top2_gap(l) <= bound
        assert int(skip.sum()) * 100 <= skip.numel(), f"{shape} {block} head {h}: {int(skip.sum())} of {skip.numel()} rows inside {bound:.3e}"
        use.append(~skip)
    return use, [_first_argmax(l) for l in l64]


# ---- 1. two-headed predict() on all four classes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("block", ["GraphSAGE", "GAT"])
@pytest.mark.parametrize("shape", SHAPES)
def test_two_headed_predict_equals_the_argmax_of_forward(shape, block):
    net = two_head_model(shape, block, seed=SHAPES.index(shape))
    gs = graphs_of(shape, 4, seed=11 + SHAPES.index(shape))
    batch = host_batch(shape, gs, [0, 1, 2, 3] if shape != "hetero" else [0, 1, 2])
    use = None
    if shape.startswith("homog"):
        use, ora_pred = oracle_compared_rows(shape, block, net, batch)  # the cap is asserted before the model runs
    net = net.to(DEV).eval()
    want = [_first_argmax(o) for o in eval_outputs(net, batch)]
    got = net.predict(batch)
    assert isinstance(got, tuple) and len(got) == 2
    got = [g.clone() for g in got]
    for h in range(2):
        assert got[h].dtype == torch.int64 and not got[h].is_cuda and got[h].numel() == want[h].numel(), (shape, h)
        if use is None:
            assert torch.equal(got[h], want[h]), f"{shape} {block} head {h}"
        else:
            assert torch.equal(got[h][use[h]], want[h][use[h]]), f"{shape} {block} head {h} (forward)"
            assert torch.equal(got[h][use[h]], ora_pred[h][use[h]]), f"{shape} {block} head {h} (oracle)"
    # the reference's spelling
    ref = tuple(p.argmax(dim=1).cpu() for p in net(batch))
    for h in range(2):
        sel = slice(None) if use is None else use[h]
        assert torch.equal(got[h][sel], ref[h][sel])
    if shape.startswith("homog"):  # labels in row order of the head's rows
        obj = batch.object_mask if shape == "homog_htree" else ~batch.room_mask
        assert got[0].numel() == int(batch.room_mask.sum()) and got[1].numel() == int(obj.sum())
        lab = net.predict_labels(batch)
        assert torch.equal(lab[0].cpu() == -1, ~batch.room_mask.cpu()) and torch.equal(lab[1].cpu() == -1, ~obj.cpu())
        assert torch.equal(lab[0][batch.room_mask].cpu(), got[0]) and torch.equal(lab[1][obj].cpu(), got[1])


@pytest.mark.parametrize("block", ["GCN", "GIN"])
def test_two_headed_op_path_predicts_what_forward_predicts(block):
    torch.manual_seed(3)
    net = HomogeneousNetwork(input_dim=6, output_dim_dict={"room": 15, "object": 35}, conv_block=block, hidden_dim=32, num_layers=3).to(DEV).eval()
    batch = host_batch("homog", graphs_of("homog", 4, 15), [0, 1, 2, 3])
    want = [_first_argmax(o) for o in eval_outputs(net, batch)]
    got = net.predict(batch)
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    lab = net.predict_labels(batch)
    assert torch.equal(lab[0].cpu() == -1, ~batch.room_mask.cpu()) and torch.equal(lab[1].cpu() == -1, batch.room_mask.cpu())
    assert torch.equal(lab[0][batch.room_mask].cpu(), want[0]) and torch.equal(lab[1][~batch.room_mask].cpu(), want[1])


# ---- 2. the latent disagreement ---------------------------------------------------------------------------------------------------
def test_all_negative_room_rows_predict_class_0_as_forward_does():
    """every room logit negative: forward()'s ReLU makes the row zero and the first index wins; the argmax of the raw state (what
    predict() returned for these nets before it knew the tail) is some other class"""
    net = two_head_model("hetero", "GraphSAGE", seed=5)
    last = f"convs.{net.num_layers - 1}."
    hit = 0
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.startswith(last) and name.endswith("__rooms.lin_l.bias"):
                p.fill_(-1.0e4)
                hit += 1
    assert hit > 0
    net = net.to(DEV).eval()
    batch = host_batch("hetero", graphs_of("hetero", 3, 21), [0, 1, 2])
    rooms_out, objects_out = eval_outputs(net, batch)
    assert float(rooms_out.abs().max()) == 0.0  # the premise: forward() sees rows of zeros
    raw = net.native().forward(batch, False)[0].cpu()
    assert bool((_first_argmax(raw[:, :26]) != 0).any())  # ... and the raw state does not point at class 0
    rooms, objects = net.predict(batch)
    assert rooms.numel() == rooms_out.size(0) and bool((rooms == 0).all())
    assert torch.equal(objects, _first_argmax(objects_out))


# ---- 3. room task -----------------------------------------------------------------------------------------------------------------
def homog_htree_room_graphs(n, seed):
    npz = np.load(workloads.HTREE_FIXTURE)
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for i in range(n):
        d = heterogeneous_htree_to_homogeneous(workloads.htree_graph(npz, i % int(npz["n_graphs"]), rng))
        del d.__dict__["edge_type"]
        out.append(d)
    return out


def room_case(name):
    """(model, per-graph data, collate function) of a room-task case"""
    torch.manual_seed(7)
    rng = np.random.default_rng(17)
    if name == "hetero":
        return (HeterogeneousNetwork({"objects": 306, "rooms": 6}, output_dim=26, conv_block="GraphSAGE", hidden_dim=32, num_layers=3),
                [workloads.mp3d_like_graph(rng) for _ in range(10)], collate)
    if name == "hetero_htree":
        npz = np.load(workloads.HTREE_FIXTURE)
        r = np.random.Generator(np.random.PCG64(18))
        return (HeterogeneousNeuralTreeNetwork(dict(HT_DIMS), output_dim=26, conv_block="GAT", disable_initialization=True, **GAT3),
                [workloads.htree_graph(npz, i % int(npz["n_graphs"]), r) for i in range(10)], collate)
    if name == "homog_htree":
        return (HomogeneousNeuralTreeNetwork(input_dim=306, output_dim=26, conv_block="GraphSAGE", hidden_dim=16, num_layers=2,
                                             disable_initialization=True), homog_htree_room_graphs(10, 19), collate_homogeneous)
    block = {"homog": "GraphSAGE", "gcn": "GCN", "gin": "GIN"}[name]
    return (HomogeneousNetwork(input_dim=6, output_dim=15, conv_block=block, hidden_dim=16, num_layers=3),
            [workloads.stanford_like_graph(rng) for _ in range(10)], collate_homogeneous)


@pytest.mark.parametrize("name", ["hetero", "hetero_htree", "homog", "homog_htree", "gcn", "gin"])
def test_room_task_predict_labels_equals_predict(name):
    net, gs, coll = room_case(name)
    net = net.to(DEV).eval()
    batch = coll(gs[:4]).to(DEV)
    want = net.predict(batch).clone()
    lab = net.predict_labels(batch)
    assert lab.is_cuda and lab.dtype == torch.int64
    if coll is collate:
        assert torch.equal(lab.cpu(), want)
    else:  # a row per node: the room label on the rows of room_mask, -1 exactly elsewhere
        rm = batch.room_mask
        assert lab.numel() == rm.numel() and torch.equal(lab.cpu() == -1, ~rm.cpu()) and torch.equal(lab[rm].cpu(), want)
    # out=: the caller's buffer is written and a view of it returned; bad buffers are refused
    buf = torch.full((lab.numel() + 5,), -7, dtype=torch.int64, device=DEV)
    view = net.predict_labels(batch, out=buf)
    assert view.data_ptr() == buf.data_ptr() and torch.equal(view, lab) and bool((buf[lab.numel():] == -7).all())
    for bad in (buf[:lab.numel() - 1], buf.to(torch.int32), buf[::2], buf.cpu()):
        with pytest.raises(_lib.HydraMPError):
            net.predict_labels(batch, out=bad)


# ---- 4. streams -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["hetero", "homog_htree", "room_node"])
def test_stream_batches_predict_what_collated_batches_predict(shape):
    if shape == "room_node":
        net, gs, _ = room_case("homog")
        net = net.to(DEV).eval()
        store = GraphStore(gs, DEV)
        stream = store.stream(net, 4, label_type="node")
    else:
        net = two_head_model(shape, "GraphSAGE", seed=9).to(DEV).eval()
        gs = graphs_of(shape, 10, 23)
        store = GraphStore(gs, DEV)
        stream = store.stream(net, 4)
    for ids in ([0, 1, 2, 5], [7], [4, 4, 9, 3], [2, 3, 6]):
        got = net.predict_labels(stream.next(ids))
        want = net.predict_labels(store.collate(ids))
        got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
        assert len(got) == len(want) == (1 if shape == "room_node" else 2)
        for g, w in zip(got, want):
            assert g.numel() > 0 and torch.equal(g, w), (shape, ids)
    # a descriptor of another model's stream is refused
    other = (room_case("homog")[0] if shape == "room_node" else two_head_model(shape, "GraphSAGE", seed=9)).to(DEV).eval()
    with pytest.raises(_lib.HydraMPError, match="another model"):
        other.predict_labels(stream.next([0, 1]))
    with pytest.raises(_lib.HydraMPError, match="another model"):
        evaluate.predict(other, (stream, [[0, 1]]))


# ---- 5. launch budget -------------------------------------------------------------------------------------------------------------
def launches(net, fn):
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


@pytest.mark.parametrize("shape", SHAPES + ("room",))
def test_predict_enqueues_the_launches_of_the_count(shape):
    if shape == "room":
        net, gs, coll = room_case("hetero")
        net = net.to(DEV).eval()
        batch = coll(gs[:4]).to(DEV)
        count = lambda: net.count_correct_rooms(batch, torch.zeros(2, dtype=torch.int64, device=DEV))  # noqa: E731
        view = batch
    else:
        net = two_head_model(shape, "GraphSAGE", seed=13).to(DEV).eval()
        batch = host_batch(shape, graphs_of(shape, 4, 29), [0, 1, 2, 3])
        counts = torch.zeros(4, dtype=torch.int64, device=DEV)
        if shape.startswith("homog"):
            count = lambda: net.count_correct(batch, "test_mask", counts)  # noqa: E731
            view = net._view(batch)
        else:
            types = net.native().head_label_types()
            count = lambda: net.count_correct(batch, tuple(batch[t].y for t in types), tuple(batch[t].test_mask for t in types), counts)  # noqa: E731
            view = batch
    n_pred = launches(net, lambda: net.predict_labels(batch))
    n_count = launches(net, count)
    n_fwd = launches(net, lambda: net.native().forward(view, False))
    print(shape, "predict", n_pred, "count", n_count, "forward", n_fwd)
    assert n_pred == n_count
    assert n_pred == [v + (1 if k == KC_LOSS else 0) for k, v in enumerate(n_fwd)]


# ---- 6. evaluate.predict ------------------------------------------------------------------------------------------------------------
class ReadCounter:
    """counts device-to-host reads: Tensor.item / cpu / tolist / numpy on a device tensor and the library's synchronising entries
    (tests/test_gpu_training_job.py::ReadCounter)"""

    TENSOR = ("item", "cpu", "tolist", "numpy")
    ENTRIES = ("hmp_epoch_read", "hmp_epoch_read_status", "hmp_net_read_state", "hmp_timer_elapsed_ms")

    def __init__(self, monkeypatch):
        self.n = 0
        self.by = {}
        lib = _lib.load()
        for name in self.TENSOR:
            monkeypatch.setattr(torch.Tensor, name, self._tensor(name, getattr(torch.Tensor, name)))
        for name in self.ENTRIES:
            monkeypatch.setattr(lib, name, self._entry(name, getattr(lib, name)))

    def _hit(self, name):
        self.n += 1
        self.by[name] = self.by.get(name, 0) + 1

    def _tensor(self, name, orig):
        def wrapped(t, *a, **k):
            if t.is_cuda:
                self._hit(name)
            return orig(t, *a, **k)

        return wrapped

    def _entry(self, name, orig):
        def wrapped(*a):
            self._hit(name)
            return orig(*a)

        return wrapped


@pytest.mark.parametrize("shape", ["hetero", "hetero_htree", "homog", "room_node", "room_hetero"])
def test_evaluate_predict_over_a_stream_reads_the_device_once(shape, monkeypatch):
    """10 graphs in batches of 4 (a short last batch): per-graph arrays equal predict() of the single-graph batches"""
    if shape.startswith("room"):
        net, gs, coll = room_case("homog" if shape == "room_node" else "hetero")
        net = net.to(DEV).eval()
        store = GraphStore(gs, DEV)
        stream = store.stream(net, 4, label_type="node" if shape == "room_node" else "rooms")
    else:
        net = two_head_model(shape, "GraphSAGE", seed=17).to(DEV).eval()
        gs = graphs_of(shape, 10, 31)
        coll = collate_homogeneous if shape.startswith("homog") else collate
        store = GraphStore(gs, DEV)
        stream = store.stream(net, 4)
    chunks = jobs.id_chunks(10, 4)
    assert [len(c) for c in chunks] == [4, 4, 2]
    evaluate.predict(net, (stream, chunks))  # warm
    torch.cuda.synchronize()
    with monkeypatch.context() as m:
        counter = ReadCounter(m)
        got = evaluate.predict(net, (stream, chunks))
    assert counter.n == 1, counter.by
    assert len(got) == 10
    for i, g in enumerate(got):
        want = net.predict(coll([gs[i]]).to(DEV))
        if isinstance(want, tuple):
            assert isinstance(g, tuple) and len(g) == 2
            for a, b in zip(g, want):
                assert a.dtype == np.int64 and np.array_equal(a, b.numpy()), (shape, i)
        else:
            assert g.dtype == np.int64 and np.array_equal(g, want.numpy()), (shape, i)
    # the iterable form: one entry per batch, the per-row vectors of predict_labels
    per_batch = evaluate.predict(net, [store.collate(ids) for ids in chunks])
    assert len(per_batch) == 3
    for ids, p in zip(chunks, per_batch):
        lab = net.predict_labels(store.collate(ids))
        for a, b in zip(p if isinstance(p, tuple) else (p,), lab if isinstance(lab, tuple) else (lab,)):
            assert np.array_equal(a, b.cpu().numpy())


# ---- 7. jobs ------------------------------------------------------------------------------------------------------------------------
class _Info:
    def __init__(self, features, rooms, objects):
        self._f, self._r, self._o = features, rooms, objects

    def num_node_features(self):
        return self._f

    def num_room_labels(self):
        return self._r

    def num_object_labels(self):
        return self._o


class GraphDataset:
    def __init__(self, data_type, graphs, features, rooms, objects=None):
        self._type, self.graphs, self._info = data_type, list(graphs), _Info(features, rooms, objects)

    def data_type(self):
        return self._type

    def __len__(self):
        return len(self.graphs)

    def __getitem__(self, i):
        return self.graphs[i]

    def get_data(self, i):
        return self._info


B = 8


def opt(job):
    job._update_training_params(optimization_params={"batch_size": B})


@pytest.mark.parametrize("name", ["hetero_sage", "homog_sage", "hetero_htree_gat", "homog_gcn"])
def test_semisupervised_job_predict_agrees_with_its_test_accuracy(name):
    if name == "hetero_sage":
        case = ("heterogeneous", workloads.semisupervised_graphs(20, 41), {"objects": 306, "rooms": 6}, 26, 28,
                dict(conv_block="GraphSAGE", hidden_dim=32, num_layers=3))
    elif name == "hetero_htree_gat":
        case = ("heterogeneous_htree", workloads.semisupervised_htree_graphs(20, 43), dict(HT_DIMS), 15, 35,
                dict(conv_block="GAT", disable_initialization=True, **GAT3))
    else:
        case = ("homogeneous", workloads.stanford_semisupervised_graphs(20, 42), 6, 15, 35,
                dict(conv_block="GraphSAGE" if name == "homog_sage" else "GCN", hidden_dim=32, num_layers=3))
    data_type, gs, feats, rooms, objects, params = case
    torch.manual_seed(4)
    job = jobs.SemiSupervisedTrainingJob(GraphDataset(data_type, gs, feats, rooms, objects), params)
    opt(job)
    job._net.to(DEV)
    acc = job.test(mask_name="test_mask")
    labels = job.predict()
    assert len(labels) == len(gs) and all(isinstance(p, tuple) and len(p) == 2 for p in labels)
    correct = total = 0
    for g, (pr, po) in zip(gs, labels):
        if data_type == "homogeneous":
            targets = ((g.y[g.room_mask], g.test_mask[g.room_mask], pr), (g.y[~g.room_mask], g.test_mask[~g.room_mask], po))
        else:
            t = ("rooms", "objects") if data_type == "heterogeneous" else ("room_virtual", "object_virtual")
            targets = ((g[t[0]].y, g[t[0]].test_mask, pr), (g[t[1]].y, g[t[1]].test_mask, po))
        for y, m, p in targets:
            assert p.dtype == np.int64 and p.shape == (y.numel(),)
            correct += int((torch.from_numpy(p)[m] == y[m]).sum())
            total += int(m.sum())
    assert total > 0 and acc == correct / total


@pytest.mark.parametrize("name", ["hetero", "homog", "gin"])
def test_room_job_predict_agrees_with_its_test_accuracy(name):
    rng = np.random.default_rng(31)
    if name == "hetero":
        data_type, gs, feats, rooms = "heterogeneous", [workloads.mp3d_like_graph(rng) for _ in range(30)], {"objects": 306, "rooms": 6}, 26
        params = dict(conv_block="GraphSAGE", hidden_dim=32, num_layers=3)
    else:
        data_type, gs, feats, rooms = "homogeneous", [workloads.stanford_like_graph(rng) for _ in range(30)], 6, 15
        params = dict(conv_block="GraphSAGE" if name == "homog" else "GIN", hidden_dim=32, num_layers=3)
    dd = {"train": GraphDataset(data_type, gs[:10], feats, rooms), "val": GraphDataset(data_type, gs[10:14], feats, rooms),
          "test": GraphDataset(data_type, gs[14:], feats, rooms)}
    torch.manual_seed(3)
    job = jobs.BaseTrainingJob(dd, params)
    opt(job)
    job._net.to(DEV)
    acc = job.test("test")
    labels = job.predict("test")
    assert len(labels) == 16
    ignored = job.ignored_label()
    correct = total = 0
    for g, p in zip(gs[14:], labels):
        y = g["rooms"].y if name == "hetero" else g.y[g.room_mask]
        assert p.dtype == np.int64 and p.shape == (y.numel(),)
        keep = y != ignored
        correct += int((torch.from_numpy(p)[keep] == y[keep]).sum())
        total += int(keep.sum())
    assert total > 0 and acc == correct / total


# ---- 8. training state --------------------------------------------------------------------------------------------------------------
def test_predict_labels_between_forward_and_backward_makes_the_backward_fail():
    net, gs, coll = room_case("hetero")
    net = net.to(DEV).train()
    batch = coll(gs[:3]).to(DEV)
    pred = net(batch)
    net.predict_labels(batch)
    with pytest.raises(_lib.HydraMPError):
        pred.sum().backward()


@pytest.mark.parametrize("shape", ["hetero", "homog"])
def test_predict_leaves_parameters_optimiser_state_and_the_dropout_counter_alone(shape):
    net = two_head_model(shape, "GraphSAGE", seed=19).to(DEV).train()
    gs = graphs_of(shape, 4, 37)
    batch = host_batch(shape, gs, [0, 1, 2, 3])
    step = net.semisupervised_step(lr=0.002, weight_decay=0.001, use_graph=False)

    def one_step():
        if shape == "homog":
            step(batch)
        else:
            types = net.native().head_label_types()
            step(batch, tuple(batch[t].y for t in types), tuple(batch[t].train_mask for t in types))

    one_step()
    torch.cuda.synchronize()
    before = [t.clone() for t in (step.flat, step.m, step.v, step.step_ctr)]
    state, rng_step, training = net.native().read_state(), net._rng_step, net.training
    net.predict_labels(batch)
    net.predict(batch)
    torch.cuda.synchronize()
    for a, b in zip(before, (step.flat, step.m, step.v, step.step_ctr)):
        assert torch.equal(a, b)
    assert net.native().read_state() == state and net._rng_step == rng_step and net.training == training
    one_step()  # and the step goes on
    torch.cuda.synchronize()
    assert step.steps_taken() == 2 and np.isfinite(step.loss())


# ---- 9. refused readout calls -------------------------------------------------------------------------------------------------------
READOUT_ENTRIES = ("hmp_net_count_correct2", "hmp_net_count_correct_heads", "hmp_net_count_correct_rooms",
                   "hmp_net_count_correct_rooms_by_graph", "hmp_net_predict_rooms", "hmp_net_predict2", "hmp_net_predict_heads",
                   "hmp_net_topk_rooms", "hmp_net_topk2", "hmp_net_topk_heads")


def net_of_kind(kind):
    """(training-mode model, batch of 2 graphs) of a net kind: "room" one output, "two" an aux readout, "heads" linear heads"""
    if kind == "room":
        net, gs, coll = room_case("hetero")
        return net.to(DEV).train(), coll(gs[:2]).to(DEV)
    shape = "hetero" if kind == "two" else "homog"
    return two_head_model(shape, "GraphSAGE", seed=23).to(DEV).train(), host_batch(shape, graphs_of(shape, 2, 41), [0, 1])


def readout_call(entry, net, batch, k):
    """the raw library call of ``entry`` on the model's net with valid, roomy buffers: only the net's kind or ``k`` is wrong"""
    nat = net.native()
    h = nat.make_batch(net._view(batch) if isinstance(net, HomogeneousNetwork) else batch)
    rows = sum(h.n_nodes) * 9 + 4
    lab = torch.zeros(2, rows, dtype=torch.int64, device=DEV)
    prb = torch.zeros(2, rows, dtype=torch.float32, device=DEV)
    mem = torch.ones(rows, dtype=torch.uint8, device=DEV)
    pair = lambda t: (C.c_void_p * 2)(t[0].data_ptr(), t[1].data_ptr())  # noqa: E731
    P, one, members = nat.flat_params(full_check=False).data_ptr(), lab[0].data_ptr(), (C.c_void_p * 2)(mem.data_ptr(), None)
    args = {"hmp_net_count_correct2": (C.byref(_lib.HeadTargets()), P, one),
            "hmp_net_count_correct_heads": (C.byref(_lib.LinearHeadTargets()), P, one),
            "hmp_net_count_correct_rooms": (P, None, 25, one, None),
            "hmp_net_count_correct_rooms_by_graph": (P, None, 25, one),
            "hmp_net_predict_rooms": (P, None, one),
            "hmp_net_predict2": (P, pair(lab)),
            "hmp_net_predict_heads": (P, members, pair(lab)),
            "hmp_net_topk_rooms": (P, None, k, one, prb[0].data_ptr()),
            "hmp_net_topk2": (P, k, pair(lab), pair(prb)),
            "hmp_net_topk_heads": (P, members, k, pair(lab), pair(prb))}[entry]
    keep = (h, lab, prb, mem)
    return lambda: (keep, getattr(nat._lib, entry)(nat._handle, C.byref(h.c), *args, _lib.stream_ptr()))[1]


@pytest.mark.parametrize("entry", READOUT_ENTRIES)
def test_a_refused_readout_call_launches_nothing_and_leaves_the_forward_usable(entry):
    """Every readout entry checks its arguments before its forward: on a net of a kind it does not serve (and, top-k, on its own
    kind with k out of range) the call fails naming the entry, enqueues no launch of any kernel class, and the backward of the
    training-mode forward before it gives the gradients, bit for bit, of a twin model that never made the call."""
    right = "room" if entry.endswith("_rooms") or entry.endswith("_by_graph") else "two" if entry.endswith("2") else "heads"
    scenarios = [("two" if right == "room" else "room", 1)]
    if "topk" in entry:
        scenarios += [(right, 0), (right, 9)]
    total = lambda out: sum(o.sum() for o in out) if isinstance(out, tuple) else out.sum()  # noqa: E731
    for kind, k in scenarios:
        (net, batch), (twin, _) = net_of_kind(kind), net_of_kind(kind)
        out, ref = net(batch), twin(batch)
        call = readout_call(entry, net, batch, k)

        def refused():
            with pytest.raises(_lib.HydraMPError, match=entry + ":"):
                _lib.check(call())

        assert launches(net, refused) == [0] * _lib.N_KCLASS, (kind, k)
        total(out).backward()
        total(ref).backward()
        torch.cuda.synchronize()
        compared = 0
        for (name, p), q in zip(net.named_parameters(), twin.parameters()):
            assert (p.grad is None) == (q.grad is None), (kind, k, name)
            if p.grad is not None:
                assert torch.equal(p.grad, q.grad), (kind, k, name)
                compared += int(bool((p.grad != 0).any()))
        assert compared > 0, (kind, k)
