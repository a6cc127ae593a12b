"""Per-graph validation counts: ``hmp_count_correct_rows_by_graph`` (operator), ``count_correct_rooms_per_graph`` (the four model
classes and a GCN model) and ``BaseTrainingJob.test_individual_graph`` -- the arithmetic of ``base_training_job.py:315-339`` for a
whole batch per launch.  Everything compared here is an integer."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hydra_gnn_amd import _lib, jobs, ops, workloads  # noqa: E402
from hydra_gnn_amd.data import heterogeneous_htree_to_homogeneous  # noqa: E402
from hydra_gnn_amd.models import (HeterogeneousNetwork, HeterogeneousNeuralTreeNetwork, HomogeneousNetwork,  # noqa: E402
                                  HomogeneousNeuralTreeNetwork)
from hydra_gnn_amd.store import GraphStore  # noqa: E402

DEV = "cuda:0"
IGNORED = 25
HT_DIMS = {"object": 306, "room": 6, "object-room": 6, "room-room": 6, "object_virtual": 306, "room_virtual": 6}


# ---- 1. the operator against a loop over graphs ---------------------------------------------------------------------------------
def loop_counts(logits, labels, members, ptr, ignored):
    C = logits.shape[1]
    pred = np.argmax(logits, axis=1)  # numpy: the first maximum
    out = np.zeros((len(ptr) - 1, 2), dtype=np.int64)
    for g in range(len(ptr) - 1):
        for r in range(ptr[g], ptr[g + 1]):
            if (members is None or members[r]) and labels[r] != ignored:
                out[g, 1] += 1
                out[g, 0] += int(0 <= labels[r] < C and pred[r] == labels[r])
    return out


@pytest.mark.parametrize("n_graphs", [1, 70])
@pytest.mark.parametrize("with_members", [False, True])
@pytest.mark.parametrize("vec", [False, True])
@pytest.mark.parametrize("C", [15, 26])
def test_operator_equals_a_loop_over_graphs(C, vec, with_members, n_graphs):
    rng = np.random.default_rng(1000 * C + 10 * n_graphs + 2 * vec + with_members)
    sizes = rng.integers(1, 31, size=n_graphs)
    if n_graphs > 1:
        sizes[5] = 0   # an empty graph: two equal consecutive offsets
        sizes[69] = 0  # ... and one at the end
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(ptr[-1])
    logits = rng.integers(0, 4, size=(n, C)).astype(np.float32)  # few distinct values: most rows have tied maxima
    labels = rng.integers(0, C, size=n).astype(np.int64)
    labels[rng.random(n) < 0.2] = IGNORED
    labels[rng.random(n) < 0.1] = C + 4  # outside [0, C) and not ignored (C + 4 != 25 for both class counts): total only
    whole = 0 if n_graphs == 1 else 11
    if n_graphs > 1:
        labels[ptr[whole]:ptr[whole + 1]] = IGNORED  # a graph with every label ignored
    members = rng.random(n) < 0.7 if with_members else None
    want = loop_counts(logits, labels, members, ptr, IGNORED)
    if n_graphs > 1:
        assert want[whole].tolist() == [0, 0] and want[5].tolist() == [0, 0] and (want[:, 1] > 0).sum() > 50
        assert (want[:, 0] > 0).any() and (want[:, 0] < want[:, 1]).any()
    ld = (C + 3) // 4 * 4 if vec else C
    buf = torch.zeros(n, ld, dtype=torch.float32, device=DEV)
    buf[:, :C] = torch.from_numpy(logits)
    buf[:, C:] = 100.0  # padding columns are never read as classes
    x = buf[:, :C]
    assert (x.data_ptr() % 16 == 0 and x.stride(0) % 4 == 0) == vec  # the walk the launcher picks
    counts = torch.zeros(n_graphs, 2, dtype=torch.int64, device=DEV)
    m = torch.from_numpy(members).to(DEV) if with_members else None
    for calls in (1, 2):  # a second call into the same buffer adds
        ops.count_correct_rows_by_graph(x, torch.from_numpy(labels).to(DEV), counts, torch.from_numpy(ptr).to(DEV), IGNORED, members=m)
        assert np.array_equal(counts.cpu().numpy(), calls * want), calls
    # the column sums are the batch-wide count
    flat = torch.zeros(2, dtype=torch.int64, device=DEV)
    ops.count_correct_rows(x, torch.from_numpy(labels).to(DEV), flat, IGNORED, members=m)
    assert flat.tolist() == want.sum(0).tolist()


def test_operator_refuses_bad_buffers():
    x = torch.zeros(6, 15, device=DEV)
    y = torch.zeros(6, dtype=torch.int64, device=DEV)
    ptr = torch.tensor([0, 2, 6], dtype=torch.int64, device=DEV)
    E = _lib.HydraMPError
    with pytest.raises(E, match="counts"):
        ops.count_correct_rows_by_graph(x, y, torch.zeros(3, 2, dtype=torch.int64, device=DEV), ptr)
    with pytest.raises(E, match="counts"):
        ops.count_correct_rows_by_graph(x, y, torch.zeros(2, 2, dtype=torch.int32, device=DEV), ptr)
    with pytest.raises(E, match="graph_ptr"):
        ops.count_correct_rows_by_graph(x, y, torch.zeros(2, 2, dtype=torch.int64, device=DEV), ptr.cpu())
    with pytest.raises(E, match="graph_ptr"):
        ops.count_correct_rows_by_graph(x, y, torch.zeros(2, 2, dtype=torch.int64, device=DEV), ptr.to(torch.int32))


# ---- 2. the models ----------------------------------------------------------------------------------------------------------------
def _htree_graphs(n, seed):
    npz = np.load(workloads.HTREE_FIXTURE)
    rng = np.random.Generator(np.random.PCG64(seed))
    k = int(npz["n_graphs"])
    return [workloads.htree_graph(npz, i % k, rng) for i in range(n)]


def _homog_htree_graphs(n, seed):
    out = []
    for g in _htree_graphs(n, seed):
        d = heterogeneous_htree_to_homogeneous(g)
        del d.__dict__["edge_type"]
        out.append(d)
    return out


def family(name):
    """(graphs, model, label_type of its stream or None)"""
    torch.manual_seed(11)
    rng = np.random.default_rng(12)
    if name == "hetero":
        gs = [workloads.mp3d_like_graph(rng) for _ in range(10)]
        return gs, HeterogeneousNetwork(input_dim_dict={"objects": 306, "rooms": 6}, output_dim=26, conv_block="GraphSAGE",
                                        hidden_dim=16, num_layers=2), "rooms"
    if name == "hetero_htree":
        return _htree_graphs(10, 13), HeterogeneousNeuralTreeNetwork(input_dim_dict=dict(HT_DIMS), output_dim=26, conv_block="GraphSAGE",
                                                                     hidden_dim=16, num_layers=2, disable_initialization=True), "room_virtual"
    if name == "homog":
        gs = [workloads.stanford_like_graph(rng) for _ in range(10)]
        gs[2].y[0] = IGNORED
        return gs, HomogeneousNetwork(input_dim=6, output_dim=15, conv_block="GAT", GAT_hidden_dims=[16], GAT_heads=[2, 2],
                                      GAT_concats=[True, False]), "node"
    if name == "homog_htree":
        return _homog_htree_graphs(10, 14), HomogeneousNeuralTreeNetwork(input_dim=306, output_dim=26, conv_block="GraphSAGE",
                                                                         hidden_dim=16, num_layers=2, disable_initialization=True), "node"
    assert name == "gcn"
    gs = [workloads.stanford_like_graph(rng) for _ in range(10)]
    return gs, HomogeneousNetwork(input_dim=6, output_dim=15, conv_block="GCN", hidden_dim=16, num_layers=2), None


def node_ptr(gs, ids):
    return torch.tensor(np.concatenate([[0], np.cumsum([gs[i].num_nodes for i in ids])]), dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("name", ["hetero", "hetero_htree", "homog", "homog_htree", "gcn"])
def test_models_count_per_graph_like_single_graph_calls(name):
    gs, net, label_type = family(name)
    net = net.to(DEV).eval()
    store = GraphStore(gs, DEV)
    ids = [7, 2, 2, 9, 0]
    singles = [net.count_correct_rooms(gs[i].to(DEV), None, None, IGNORED) for i in ids]
    batch = store.collate(ids)
    whole = net.count_correct_rooms(batch, None, None, IGNORED)
    print(name, "singles", singles, "batch", whole)
    assert sum(s[1] for s in singles) == whole[1] > 0
    kw = dict(graph_ptr=node_ptr(gs, ids)) if store.homogeneous else {}
    counts = torch.zeros(5, 2, dtype=torch.int64, device=DEV)
    assert net.count_correct_rooms_per_graph(batch, counts, IGNORED, **kw) is counts
    assert counts.tolist() == [list(s) for s in singles]
    assert counts.sum(0).tolist() == list(whole)
    if label_type is None:
        return
    stream = store.stream(net, 5, label_type)
    net.count_correct_rooms_per_graph(stream.next(ids), counts, IGNORED)  # adds
    assert counts.tolist() == [[2 * v for v in s] for s in singles]
    part = torch.zeros(2, 2, dtype=torch.int64, device=DEV)  # a partial batch on the same stream
    net.count_correct_rooms_per_graph(stream.next(ids[3:]), part, IGNORED)
    assert part.tolist() == [list(s) for s in singles[3:]]
    with pytest.raises(_lib.HydraMPError, match="counts"):
        net.count_correct_rooms_per_graph(stream.next(ids), part, IGNORED)


def test_a_homogeneous_batch_needs_graph_ptr_and_two_headed_models_refuse():
    gs, net, _ = family("homog")
    net = net.to(DEV).eval()
    batch = GraphStore(gs, DEV).collate([0, 1])
    counts = torch.zeros(2, 2, dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.HydraMPError, match="graph_ptr"):
        net.count_correct_rooms_per_graph(batch, counts)
    two = HomogeneousNetwork(input_dim=6, output_dim_dict={"room": 15, "object": 35}, conv_block="GraphSAGE", hidden_dim=16,
                             num_layers=2).to(DEV)
    with pytest.raises(_lib.HydraMPError, match="two-headed"):
        two.count_correct_rooms_per_graph(batch, counts, graph_ptr=node_ptr(gs, [0, 1]))


# ---- 3. the job -------------------------------------------------------------------------------------------------------------------
class _Info:
    def __init__(self, features, rooms):
        self._f, self._r = features, rooms

    def num_node_features(self):
        return self._f

    def num_room_labels(self):
        return self._r


class GraphDataset:
    def __init__(self, data_type, graphs, features, rooms):
        self._type, self.graphs, self._info = data_type, list(graphs), _Info(features, rooms)

    def data_type(self):
        return self._type

    def __len__(self):
        return len(self.graphs)

    def __getitem__(self, i):
        return self.graphs[i]

    def get_data(self, i):
        return self._info


class ReadCounter:
    """device-to-host reads, counted as tests/test_gpu_training_job.py counts them: Tensor.item / cpu / tolist / numpy on a device
    tensor and the library's synchronising entries"""

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


def make_job(name):
    rng = np.random.default_rng(21)
    if name == "hetero_sage":
        data_type, gs, feats, rooms = "heterogeneous", [workloads.mp3d_like_graph(rng) for _ in range(14)], {"objects": 306, "rooms": 6}, 26
        params = dict(conv_block="GraphSAGE", hidden_dim=16, num_layers=2)
    elif name == "homog_htree_sage":
        data_type, gs, feats, rooms = "homogeneous_htree", _homog_htree_graphs(14, 22), 306, 26
        params = dict(conv_block="GraphSAGE", hidden_dim=16, num_layers=2, disable_initialization=True)
    else:
        data_type, gs, feats, rooms = "homogeneous", [workloads.stanford_like_graph(rng) for _ in range(14)], 6, 15
        gs[12].y[0] = IGNORED
        params = dict(conv_block={"homog_sage": "GraphSAGE", "gin": "GIN"}[name], hidden_dim=16, num_layers=2)
    dd = {s: GraphDataset(data_type, gs[:4], feats, rooms) for s in ("train", "val", "test")}
    torch.manual_seed(23)
    job = jobs.BaseTrainingJob(dd, params)
    job._update_training_params(optimization_params={"batch_size": 4})  # 10 graphs: two full batches and a partial one
    return job, GraphDataset(data_type, gs[4:], feats, rooms)


@pytest.mark.parametrize("name", ["hetero_sage", "homog_sage", "homog_htree_sage", "gin"])
def test_job_counts_individual_graphs_in_batches_and_reads_once(name, monkeypatch):
    job, dataset = make_job(name)
    net = job._net.to(DEV).eval()
    want = [tuple(net.count_correct_rooms(g.to(DEV), None, None, IGNORED)) for g in dataset.graphs]
    assert len(want) == 10
    with monkeypatch.context() as m:
        counter = ReadCounter(m)
        got = job.test_individual_graph(dataset)
    print(name, got, counter.by)
    assert got == want and all(isinstance(v, int) for pair in got for v in pair)
    assert counter.n == 1, counter.by
    if name != "gin":
        assert job.test_individual_graph(dataset) == want  # the uploaded copy and its stream are reused
        assert job._stores["individual"][1] is dataset
    assert job.test_individual_graph(GraphDataset(dataset.data_type(), [], 0, 0)) == []
