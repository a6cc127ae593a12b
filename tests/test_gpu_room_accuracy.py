"""GPU checks of the room-task validation count (csrc/evaluate.hip, hmp_count_correct_rows / hmp_net_count_correct_rooms): the
operator against torch argmax + bincount, every model family against the arithmetic of BaseTrainingJob.test
(base_training_job.py:269-313) on ``model.eval(); model(data)``, eval counts interleaved with training steps, BatchStream batches
and ``evaluate.accuracy``.  Every comparison is exact integer equality."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hydra_gnn_amd import _lib, evaluate, ops, workloads  # noqa: E402
from hydra_gnn_amd.data import collate, collate_homogeneous  # noqa: E402
from hydra_gnn_amd.models import (HeterogeneousNetwork, HeterogeneousNeuralTreeNetwork, HomogeneousNetwork,  # noqa: E402
                                  HomogeneousNeuralTreeNetwork)
from hydra_gnn_amd.store import GraphStore  # noqa: E402

DEV = "cuda:0"
HT_DIMS = {"object": 306, "room": 6, "object-room": 6, "room-room": 6, "object_virtual": 306, "room_virtual": 6}


# ---- the reference's arithmetic ---------------------------------------------------------------------------------------------
def ref_test(pred_batches, label_batches, ignored, C):
    """BaseTrainingJob.test's loop body (base_training_job.py:283-308) on host tensors: (correct, total, accuracy_matrix), the
    matrix summed over the batches (the reference assigns it per batch; equal for one batch)"""
    correct = total = 0
    mat = np.zeros((C - 1, C), dtype=int)
    for pred, label in zip(pred_batches, label_batches):
        mask = label != ignored
        pred, label = pred[mask], label[mask]
        correct += pred.eq(label).sum().item()
        total += torch.numel(label)
        for l in range(C - 1):
            if l == ignored:
                continue
            for ll in range(C):
                mat[l, ll] += (pred[label == l] == ll).sum().item()
    return correct, total, mat


def torch_counts(logits, labels, ignored, members, C):
    """counts and [C, C] confusion matrix from torch.argmax + bincount"""
    pred = logits.argmax(dim=1)
    keep = labels != ignored
    if members is not None:
        keep &= members
    p, l = pred[keep], labels[keep]
    inr = (l >= 0) & (l < C)
    conf = torch.bincount(l[inr] * C + p[inr], minlength=C * C)
    return [int((p == l).sum()), int(keep.sum())], conf


# ---- 1. the operator --------------------------------------------------------------------------------------------------------
def tie_logits(n, C, ld, seed):
    """[n, C] view of an [n, ld] buffer: small integers (many exact ties), some rows constant (every column ties)"""
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((max(n, 1), ld), 7.0)
    buf[:, :C] = torch.randint(-3, 4, (max(n, 1), C), generator=g).float()
    if n > 2:
        buf[::7, :C] = 1.5  # whole-row ties: the first column wins
        buf[1, :C] = -2.0
    return buf[:n, :C]


@pytest.mark.parametrize("C", [1, 3, 4, 15, 17, 26, 33, 64, 65, 130])
@pytest.mark.parametrize("n", [0, 1, 17, 5003])
def test_operator_matches_torch_argmax_and_bincount(C, n):
    ignored = 25 if C > 25 else C // 2
    lds = sorted({C, (C + 3) // 4 * 4, C + 1, (C + 3) // 4 * 4 + 4})  # unit, quad-padded (16-byte loads), odd pitch
    g = torch.Generator().manual_seed(C * 7 + n)
    labels = torch.randint(-2, C + 2, (n,), generator=g)
    labels[::5] = ignored
    members = torch.rand(n, generator=g) < 0.7
    for ld in lds:
        host = tie_logits(n, C, ld, seed=ld + n)
        logits = torch.as_strided(_padded(host, ld), (n, C), (ld, 1)) if n else torch.zeros(0, C, device=DEV)
        assert logits.stride(0) == ld or n <= 1
        pred_dev = ops.argmax_rows(logits).cpu()  # hmp_argmax_rows
        assert torch.equal(pred_dev, host.argmax(dim=1))
        for mem in (None, members):
            want, conf_want = torch_counts(host, labels, ignored, mem, C)
            counts = torch.zeros(2, dtype=torch.int64, device=DEV)
            conf = torch.zeros(C, C, dtype=torch.int64, device=DEV)
            for k in (1, 2):  # two calls accumulate
                ops.count_correct_rows(logits, labels.to(DEV), counts, ignored_label=ignored,
                                       members=mem.to(DEV) if mem is not None else None, confusion=conf)
                assert counts.cpu().tolist() == [k * v for v in want], (ld, mem is None, k)
                assert torch.equal(conf.cpu().reshape(-1), k * conf_want), (ld, mem is None, k)
            c2 = torch.zeros(2, dtype=torch.int64, device=DEV)
            ops.count_correct_rows(logits, labels.to(DEV), c2, ignored_label=ignored,
                                   members=mem.to(DEV) if mem is not None else None)
            assert c2.cpu().tolist() == want
            # the confusion matrix agrees with the predictions of hmp_argmax_rows
            keep = (labels != ignored) & (mem if mem is not None else True)
            l, p = labels[keep], pred_dev[keep]
            inr = (l >= 0) & (l < C)
            assert torch.equal(conf.cpu().reshape(-1), 2 * torch.bincount(l[inr] * C + p[inr], minlength=C * C))


def _padded(host, ld):
    n, C = host.shape
    buf = torch.full((n, ld), 7.0)  # padding larger than every logit: a read past the row would change the argmax
    buf[:, :C] = host
    return buf.reshape(-1).to(DEV)


@pytest.mark.parametrize("C", [1, 3, 4, 17, 64, 65, 130])
def test_one_tie_rule_across_entries(C):
    """hmp_argmax_rows and hmp_count_correct_rows share one first-maximum rule on rows full of exact ties, whichever column walk
    the buffer's pitch selects (16-byte quads or scalar columns): a count against the other entry's predictions is all correct"""
    n = 37
    aligned, odd = (C + 3) // 4 * 4, (C + 3) // 4 * 4 + 1
    for ld in (aligned, odd):
        host = tie_logits(n, C, ld, seed=C + ld)
        logits = torch.as_strided(_padded(host, ld), (n, C), (ld, 1))
        pred = ops.argmax_rows(logits)
        assert np.array_equal(pred.cpu().numpy(), np.argmax(host.numpy(), axis=1)), ld
        counts = torch.zeros(2, dtype=torch.int64, device=DEV)
        conf = torch.zeros(C, C, dtype=torch.int64, device=DEV)
        ops.count_correct_rows(logits, pred, counts, ignored_label=-1, confusion=conf)
        assert counts.cpu().tolist() == [n, n], ld
        conf = conf.cpu()
        assert int(conf.sum()) == n and int(conf.diagonal().sum()) == n, ld
        assert torch.equal(conf.diagonal(), torch.bincount(pred.cpu(), minlength=C)), ld


def test_operator_strides_over_many_rows_and_flags_nothing_else():
    """more rows than the capped grid covers in one pass (the workgroups stride), NaN-free random floats"""
    n, C = 40_011, 26
    g = torch.Generator().manual_seed(3)
    host = torch.randn(n, C, generator=g)
    labels = torch.randint(0, C, (n,), generator=g)
    counts = torch.zeros(2, dtype=torch.int64, device=DEV)
    conf = torch.zeros(C * C, dtype=torch.int64, device=DEV)
    ops.count_correct_rows(host.to(DEV), labels.to(DEV), counts, ignored_label=25, confusion=conf)
    want, conf_want = torch_counts(host, labels, 25, None, C)
    assert counts.cpu().tolist() == want and torch.equal(conf.cpu(), conf_want)


def test_operator_refuses_bad_buffers():
    x = torch.zeros(4, 5, device=DEV)
    y = torch.zeros(4, dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.HydraMPError):
        ops.count_correct_rows(x, y, torch.zeros(2, dtype=torch.int32, device=DEV))
    with pytest.raises(_lib.HydraMPError):
        ops.count_correct_rows(x, y, torch.zeros(2, dtype=torch.int64, device=DEV), confusion=torch.zeros(24, dtype=torch.int64, device=DEV))
    with pytest.raises(_lib.HydraMPError):
        ops.count_correct_rows(x, y, torch.zeros(2, dtype=torch.int64, device=DEV), members=torch.ones(4, dtype=torch.uint8, device=DEV))


# ---- 2. every model family against test()'s arithmetic ----------------------------------------------------------------------
def _with_ignored(y, every=4):
    y = y.clone()
    y[::every] = 25
    return y


def mp3d_batch(B, seed, rel_pos=False):
    b = workloads.mp3d_like_batch(B, seed=seed, relative_pos=rel_pos)
    b["rooms"].y = _with_ignored(b["rooms"].y)
    return b


def check_family(model, batch, labels_of, C):
    model = model.to(DEV).eval()
    gb = batch.to(DEV)
    with torch.no_grad():
        pred = model(gb).argmax(dim=1).cpu()
    label = labels_of(batch)
    correct, total, mat = ref_test([pred], [label], 25, C)
    assert total > 0
    assert model.count_correct_rooms(gb) == [correct, total]
    counts = torch.zeros(2, dtype=torch.int64, device=DEV)
    conf = torch.zeros(C, C, dtype=torch.int64, device=DEV)
    for _ in range(2):
        model.count_correct_rooms(gb, counts, conf)
    assert counts.cpu().tolist() == [2 * correct, 2 * total]
    assert np.array_equal(evaluate.accuracy_matrix(conf, 25), 2 * mat)
    acc, m1 = evaluate.accuracy(model, [gb], per_label=True)
    assert acc == correct / total and np.array_equal(m1, mat)
    return correct, total


HET_KW = dict(input_dim_dict={"objects": 306, "rooms": 6}, output_dim=26, hidden_dim=32, num_layers=3, GAT_hidden_dims=[16, 16],
              GAT_heads=[2, 2, 2], GAT_concats=[True, True, False], dropout=0.25)


@pytest.mark.parametrize("block", ["GraphSAGE", "GAT", "GAT_edge"])
def test_heterogeneous_baseline_counts_equal_test_arithmetic(block):
    torch.manual_seed(1)
    kw = dict(HET_KW, conv_block=block)
    if block == "GAT_edge":
        kw["input_dim_dict"] = {"objects": 303, "rooms": 3}
    batch = mp3d_batch(32, seed=11, rel_pos=block == "GAT_edge")
    check_family(HeterogeneousNetwork(**kw), batch, lambda b: b["rooms"].y, 26)


def test_htree_counts_equal_test_arithmetic():
    torch.manual_seed(2)
    net = HeterogeneousNeuralTreeNetwork(HT_DIMS, output_dim=26, conv_block="GraphSAGE", hidden_dim=32, num_layers=3,
                                         disable_initialization=True, dropout=0.25)
    batch = workloads.htree_batch(8, seed=12)
    batch["room_virtual"].y = _with_ignored(batch["room_virtual"].y)
    check_family(net, batch, lambda b: b["room_virtual"].y, 26)


def stanford_batch(n_graphs, seed):
    rng = np.random.Generator(np.random.PCG64(workloads.BASE_SEED + seed))
    b = collate_homogeneous([workloads.stanford_like_graph(rng) for _ in range(n_graphs)])
    b.y = _with_ignored(b.y, every=3)
    return b


@pytest.mark.parametrize("block", ["GraphSAGE", "GCN", "GIN"])
def test_homogeneous_counts_equal_test_arithmetic(block):
    torch.manual_seed(3)
    net = HomogeneousNetwork(input_dim=6, output_dim=15, conv_block=block, hidden_dim=32, num_layers=3, dropout=0.25)
    b = stanford_batch(24, seed=5)
    b.y[b.room_mask] = _with_ignored(b.y[b.room_mask], every=3)  # rows outside room_mask keep labels: members must drop them
    check_family(net, b, lambda d: d.y[d.room_mask], 15)
    if block == "GIN":
        assert [int(bn.module.num_batches_tracked) for bn in net.batch_norms] == [0, 0, 0]


def homogeneous_htree_batch(n_graphs, seed):
    from hydra_gnn_amd.data import heterogeneous_htree_to_homogeneous

    npz = np.load(workloads.HTREE_FIXTURE)
    rng = np.random.Generator(np.random.PCG64(seed))
    n = int(npz["n_graphs"])
    graphs = []
    for i in range(n_graphs):
        d = heterogeneous_htree_to_homogeneous(workloads.htree_graph(npz, i % n, rng))
        del d.__dict__["edge_type"]
        graphs.append(d)
    b = collate_homogeneous(graphs)
    b.y[b.room_mask] = _with_ignored(b.y[b.room_mask], every=3)
    return b


@pytest.mark.parametrize("block", ["GraphSAGE", "GCN"])
def test_homogeneous_htree_counts_equal_test_arithmetic(block):
    torch.manual_seed(4)
    net = HomogeneousNeuralTreeNetwork(306, output_dim=26, conv_block=block, hidden_dim=32, num_layers=3,
                                       disable_initialization=True, dropout=0.25)
    check_family(net, homogeneous_htree_batch(4, seed=13), lambda d: d.y[d.room_mask], 26)


def test_two_headed_models_refuse_and_existing_refusal_stays():
    net = HeterogeneousNetwork({"objects": 306, "rooms": 6}, output_dim_dict={"rooms": 26, "objects": 10},
                               conv_block="GraphSAGE", hidden_dim=16, num_layers=2).to(DEV)
    with pytest.raises(_lib.HydraMPError, match="count_correct"):
        net.count_correct_rooms(workloads.semisupervised_batch(2, seed=1).to(DEV))
    room = HeterogeneousNetwork(**dict(HET_KW, conv_block="GraphSAGE")).to(DEV)
    with pytest.raises(_lib.HydraMPError):
        room.count_correct(mp3d_batch(2, seed=1).to(DEV), (None, None))


# ---- 3. eval leaves training alone ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [True, False])
def test_eval_between_steps_leaves_training_bit_identical(use_graph):
    kw = dict(HET_KW, conv_block="GraphSAGE")
    torch.manual_seed(5)
    net_a = HeterogeneousNetwork(**kw).to(DEV)
    torch.manual_seed(5)
    net_b = HeterogeneousNetwork(**kw).to(DEV)
    train = mp3d_batch(16, seed=21).to(DEV)
    val = mp3d_batch(8, seed=22).to(DEV)
    y = train["rooms"].y
    step_a = net_a.train_step(lr=0.002, weight_decay=0.001, ignored_label=25, seed=9, use_graph=use_graph)
    step_b = net_b.train_step(lr=0.002, weight_decay=0.001, ignored_label=25, seed=9, use_graph=use_graph)
    counts = torch.zeros(2, dtype=torch.int64, device=DEV)
    for it in range(6):
        step_a(train, y)
        flat = net_a.native().flat_params(full_check=False).clone()
        net_a.count_correct_rooms(val, counts)
        assert torch.equal(net_a.native().flat_params(full_check=False), flat), "an eval changed the parameters"
        step_b(train, y)
        assert step_a.loss() == step_b.loss(), it
    assert torch.equal(step_a.m, step_b.m) and torch.equal(step_a.v, step_b.v)
    for (n, p), (_, q) in zip(net_a.named_parameters(), net_b.named_parameters()):
        assert torch.equal(p, q), n
    assert step_a.steps_taken() == step_b.steps_taken() == 6
    assert int(counts[1]) == 6 * int((val["rooms"].y != 25).sum())


def test_backward_after_an_eval_count_is_refused():
    torch.manual_seed(6)
    net = HeterogeneousNetwork(**dict(HET_KW, conv_block="GraphSAGE")).to(DEV).train()
    b = mp3d_batch(4, seed=23).to(DEV)
    out = net(b)
    net.count_correct_rooms(b)
    with pytest.raises(_lib.HydraMPError, match="backward"):
        out.sum().backward()


# ---- 4. stream batches ------------------------------------------------------------------------------------------------------
def _mp3d_graphs(n, seed):
    rng = np.random.default_rng(seed)
    gs = [workloads.mp3d_like_graph(rng) for _ in range(n)]
    for g in gs[::3]:
        g["rooms"].y[0] = 25
    return gs


def _htree_graphs(n, seed):
    npz = np.load(workloads.HTREE_FIXTURE)
    rng = np.random.Generator(np.random.PCG64(seed))
    k = int(npz["n_graphs"])
    gs = [workloads.htree_graph(npz, i % k, rng) for i in range(n)]
    for g in gs[::3]:
        g["room_virtual"].y[0] = 25
    return gs


@pytest.mark.parametrize("family", ["baseline", "htree"])
def test_stream_batches_count_like_collated_batches(family):
    def make():
        torch.manual_seed(7)
        if family == "baseline":
            return HeterogeneousNetwork(**dict(HET_KW, conv_block="GraphSAGE")).to(DEV)
        return HeterogeneousNeuralTreeNetwork(HT_DIMS, output_dim=26, conv_block="GraphSAGE", hidden_dim=32, num_layers=3,
                                              disable_initialization=True, dropout=0.25).to(DEV)

    gs, label_type = (_mp3d_graphs(48, seed=8), "rooms") if family == "baseline" else (_htree_graphs(24, seed=8), "room_virtual")
    net, net_ref = make(), make()
    net.eval()
    store = GraphStore(gs, DEV)
    B = 8
    stream = store.stream(net, B, label_type)
    rng = np.random.default_rng(9)
    id_lists = [rng.choice(len(gs), size=B if i % 3 else B // 2, replace=False).tolist() for i in range(7)]
    counts = torch.zeros(2, dtype=torch.int64, device=DEV)
    conf = torch.zeros(26 * 26, dtype=torch.int64, device=DEV)
    for ids in id_lists:
        net.count_correct_rooms(stream.next(ids), counts, conf)
    want = torch.zeros(2, dtype=torch.int64, device=DEV)
    conf_want = torch.zeros(26 * 26, dtype=torch.int64, device=DEV)
    preds, labels = [], []
    for ids in id_lists:
        b = collate([gs[i] for i in ids]).to(DEV)
        net.count_correct_rooms(b, want, conf_want)
        with torch.no_grad():
            preds.append(net(b).argmax(dim=1).cpu())
        labels.append(b[label_type].y.cpu())
    assert torch.equal(counts, want) and torch.equal(conf, conf_want)
    correct, total, mat = ref_test(preds, labels, 25, 26)
    assert counts.cpu().tolist() == [correct, total]
    assert np.array_equal(evaluate.accuracy_matrix(conf, 25), mat)
    assert evaluate.accuracy(net, (stream, id_lists)) == correct / total
    assert net.native().read_state()[1] == 0

    # training steps and eval batches on the same stream
    step = net.train_step(lr=0.002, weight_decay=0.001, ignored_label=25, seed=3, use_graph=False)
    step_ref = net_ref.train_step(lr=0.002, weight_decay=0.001, ignored_label=25, seed=3, use_graph=False)
    c2 = torch.zeros(2, dtype=torch.int64, device=DEV)
    for i, ids in enumerate(id_lists):
        step.run(stream.next(ids))
        b = collate([gs[j] for j in ids]).to(DEV)
        step_ref(b, b[label_type].y)
        assert step.loss() == step_ref.loss(), i
        net.count_correct_rooms(stream.next(id_lists[-1 - i]), c2)
    for (n, p), (_, q) in zip(net.named_parameters(), net_ref.named_parameters()):
        assert torch.equal(p, q), n
    stream.close()


def test_stream_batch_refuses_extra_labels():
    gs = _mp3d_graphs(8, seed=10)
    net = HeterogeneousNetwork(**dict(HET_KW, conv_block="GraphSAGE")).to(DEV)
    stream = GraphStore(gs, DEV).stream(net, 4, "rooms")
    h = stream.next([0, 1, 2, 3])
    with pytest.raises(_lib.HydraMPError, match="labels"):
        net.native().count_correct_rooms(h, torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV))
    stream.close()


# ---- 5. evaluate.accuracy over a loader -------------------------------------------------------------------------------------
def test_accuracy_over_a_loader_equals_reference_test():
    torch.manual_seed(8)
    net = HeterogeneousNetwork(**dict(HET_KW, conv_block="GraphSAGE")).to(DEV)
    gs = _mp3d_graphs(40, seed=14)
    loader = [collate(gs[i:i + 8]).to(DEV) for i in range(0, 40, 8)]
    net.eval()
    with torch.no_grad():
        preds = [net(b).argmax(dim=1).cpu() for b in loader]
    labels = [b["rooms"].y.cpu() for b in loader]
    correct, total, mat = ref_test(preds, labels, 25, 26)
    assert evaluate.accuracy(net, loader) == correct / total
    acc, m = evaluate.accuracy(net, loader, per_label=True)
    assert acc == correct / total and np.array_equal(m, mat)
    # one batch: the reference's matrix itself (its loop assigns the last batch's matrix)
    c1, t1, m1 = ref_test(preds[-1:], labels[-1:], 25, 26)
    acc1, mm1 = evaluate.accuracy(net, loader[-1:], per_label=True)
    assert acc1 == c1 / t1 and np.array_equal(mm1, m1)
