"""Fused step of the homogeneous two-headed (room + object) task: ``HomogeneousNetwork`` / ``HomogeneousNeuralTreeNetwork`` with
``output_dim_dict`` train through ``semisupervised_step`` (the loop body of the reference's ``SemiSupervisedTrainingJob.train``,
semisupervised_training_job.py:117-147, homogeneous branches: two learned ``nn.Linear`` heads over rows of one node set) and
count through ``count_correct`` (its ``test()``, :198-257).  The step must equal the ``loss.backward()`` loop on the same engine
(same dropout masks), the oracle in float64, and the data-parallel protocol of the other fused steps."""
import copy
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hydra_gnn_amd import _lib, workloads  # noqa: E402
from hydra_gnn_amd.data import collate_homogeneous  # noqa: E402
from hydra_gnn_amd.models import HomogeneousNetwork, HomogeneousNeuralTreeNetwork  # noqa: E402
from oracle import models as omodels  # noqa: E402

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
LR, WD = 0.002, 0.001
OUT = {"room": 15, "object": 35}
GAT_KW = dict(GAT_hidden_dims=[16, 16], GAT_heads=[3, 3], GAT_concats=[True, True])


def model_kw(block, htree=False, init=False, dropout=0.25, hidden=32):
    kw = dict(input_dim=6, output_dim_dict=dict(OUT), conv_block=block, hidden_dim=hidden, num_layers=3, dropout=dropout)
    if block != "GraphSAGE":
        kw.update(GAT_KW)
    if htree:
        kw.update(disable_initialization=not init)
    return kw


def twin_nets(block, htree=False, init=False, dropout=0.25, seed=0, hidden=32):
    """two identical fresh models (same weights, same dropout seed, counters at 0)"""
    torch.manual_seed(seed)
    cls = HomogeneousNeuralTreeNetwork if htree else HomogeneousNetwork
    a = cls(**model_kw(block, htree, init, dropout, hidden))
    if htree and init:
        with torch.no_grad():
            a.pre_mp.bias.uniform_(-0.2, 0.2)
    b = copy.deepcopy(a)
    return a.to(DEV), b.to(DEV)


def with_edge_attr(batch, block, seed=3):
    if block == "GAT_edge":
        g = torch.Generator().manual_seed(seed)
        batch.edge_attr = torch.randn(batch.edge_index.size(1), 3, generator=g)
    return batch


def stanford_batch(block, n=12, seed=11):
    return with_edge_attr(workloads.stanford_semisupervised_batch(n, seed), block).to(DEV)


def htree_batch(block, n=4, seed=47):
    """H-tree graphs built like tests/test_gpu_htree.py::homogeneous_htree_batch from the committed fixture, 6-d features, per-node
    labels valid for both heads' classes on the virtual rows, a seeded train / val / test split"""
    from hydra_gnn_amd.data import heterogeneous_htree_to_homogeneous

    npz = np.load(workloads.HTREE_FIXTURE)
    rng = np.random.Generator(np.random.PCG64(seed))
    graphs = []
    for i in range(n):
        d = heterogeneous_htree_to_homogeneous(workloads.htree_graph(npz, i % int(npz["n_graphs"]), rng))
        del d.__dict__["edge_type"]
        graphs.append(d)
    b = collate_homogeneous(graphs)
    b.x = b.x[:, :6].contiguous()
    N = b.x.size(0)
    y = torch.from_numpy(rng.integers(0, OUT["object"], size=N))
    y[b.room_mask] = torch.from_numpy(rng.integers(0, OUT["room"], size=int(b.room_mask.sum())))
    b.y = y
    u = torch.from_numpy(rng.random(N))
    b.train_mask, b.val_mask, b.test_mask = u < 0.6, (u >= 0.6) & (u < 0.8), u >= 0.8
    assert int(b.object_mask.sum()) > 0 and int(b.room_mask.sum()) > 0
    assert int((~(b.room_mask | b.object_mask)).sum()) > 0  # rows in neither head
    return with_edge_attr(b, block).to(DEV)


def object_rows(net, data):
    return data.object_mask if isinstance(net, HomogeneousNeuralTreeNetwork) else ~data.room_mask


def ref_targets(net, data, mask):
    """the reference's indexed tuples (semisupervised_training_job.py:117-147)"""
    rm, om = data.room_mask, object_rows(net, data)
    return (data.y[rm], data.y[om]), (mask[rm], mask[om])


def autograd_loss(net, data, mask):
    labels, masks = ref_targets(net, data, mask)
    return net.loss(net(data), labels, masks)


def compare_params(got, ref, tiny, steps, what):
    """the tolerance scheme of tests/test_gpu_semisupervised.py: Adam-ill-conditioned elements excluded and counted"""
    n_tiny = n_all = 0
    for name, p in got.named_parameters():
        r = ref[name].detach().cpu().double()
        diff = (p.detach().cpu().double() - r).abs()
        ok = ~tiny[name]
        n_tiny += int(tiny[name].sum())
        n_all += tiny[name].numel()
        if bool(ok.any()):
            assert float(diff[ok].max()) <= 1e-3, f"{name} ({what})"
            assert float((diff[ok] > 5e-5).double().mean()) < 0.01, f"{name} ({what})"
        assert float(diff.max()) <= steps * LR * 2.1, f"{name} ({what})"
    assert n_tiny < 0.3 * n_all


CASES = [(False, False, "GraphSAGE"), (False, False, "GAT"), (False, False, "GAT_edge"),
         (True, False, "GraphSAGE"), (True, False, "GAT"), (True, False, "GAT_edge"),
         (True, True, "GraphSAGE"), (True, True, "GAT"), (True, True, "GAT_edge")]


@pytest.mark.parametrize("htree,init,block", CASES)
def test_fused_step_equals_autograd_loop(htree, init, block):
    """path A: net(data) -> net.loss(pred, indexed labels, indexed masks) -> backward -> torch.optim.Adam; path B:
    semisupervised_step, eager and graph-replayed.  Dropout 0.25 (features, the tail, GAT attention): same masks, same steps"""
    gb = htree_batch(block) if htree else stanford_batch(block)
    a, _ = twin_nets(block, htree, init)
    opt = torch.optim.Adam(a.parameters(), lr=LR, weight_decay=WD)
    tiny = {n: torch.zeros_like(p, dtype=torch.bool, device="cpu") for n, p in a.named_parameters()}
    a.train()
    losses_a = []
    for _ in range(5):
        opt.zero_grad()
        loss = autograd_loss(a, gb, gb.train_mask)
        loss.backward()
        for n, p in a.named_parameters():
            if p.grad is not None:
                tiny[n] |= (p.grad.abs() < 1e-5).cpu()
        opt.step()
        losses_a.append(float(loss))
    ref = dict(a.named_parameters())
    for use_graph in (False, True):
        _, b = twin_nets(block, htree, init)
        sd0 = {k: v.clone() for k, v in b.state_dict().items()}
        step = b.semisupervised_step(lr=LR, weight_decay=WD, use_graph=use_graph)
        assert list(b.state_dict()) == list(sd0) and all(torch.equal(b.state_dict()[k], v) for k, v in sd0.items())
        losses_b = []
        for _ in range(5):
            step(gb)
            losses_b.append(step.loss())
        np.testing.assert_allclose(losses_b, losses_a, rtol=2e-5, atol=2e-6)
        compare_params(b, ref, tiny, 5, f"{block}, htree={htree}, init={init}, graph={use_graph}")
        assert b.native().read_state() == (5, 0)
        if use_graph:
            assert step._graphs is not None and step._key is not None
            key = step._key
            step(gb)
            assert step._key == key  # the same tensors: no re-capture


def phase_a(net, data, mask=None, **kw):
    """phase A only (force_collective without a process group: A, no-op all-reduce, B at lr 0): flat SUM gradient + {loss, count}"""
    step = net.semisupervised_step(lr=0.0, use_graph=False, force_collective=True, **kw)
    step(data, mask=mask)
    torch.cuda.synchronize()
    return step


def grad_of(net, step, p):
    off = net.native().param_offsets[id(p)]
    return step.grads[off: off + p.numel()].view(p.shape)


def check_against_autograd(a, b, data, mask, **kw):
    """one step: phase A of the fused step on b == loss.backward() on the twin a (first draw of both)"""
    a.train()
    loss = autograd_loss(a, data, mask)
    loss.backward()
    step = phase_a(b, data, mask=mask, **kw)
    cnt = float(step.grads[b.native().n_active + 1])
    assert abs(step.loss() - float(loss)) <= 2e-5 * max(1.0, abs(float(loss)))
    pb = dict(b.named_parameters())
    for name, p in a.named_parameters():
        g = grad_of(b, step, pb[name]) / max(cnt, 1.0)
        if p.grad is None:
            continue
        torch.testing.assert_close(g, p.grad, atol=2e-5, rtol=1e-4, msg=lambda m: f"{name}: {m}")
    return step


def test_head_without_counted_rows_has_zero_gradient():
    gb = stanford_batch("GraphSAGE")
    _, b = twin_nets("GraphSAGE")
    mask = gb.train_mask & gb.room_mask  # no object row counts
    step = phase_a(b, gb, mask=mask)
    for p in (b.post_mp_object.weight, b.post_mp_object.bias):
        assert bool((grad_of(b, step, p) == 0).all())
    assert bool((grad_of(b, step, b.post_mp_room.weight) != 0).any())
    assert float(step.grads[b.native().n_active + 1]) == float(mask.sum())


def test_rows_in_no_head_contribute_nothing():
    """H-tree clique rows belong to neither head: their labels (even out of range) change neither the gradient nor the status"""
    gb = htree_batch("GraphSAGE")
    _, b1 = twin_nets("GraphSAGE", True)
    _, b2 = twin_nets("GraphSAGE", True)
    s1 = phase_a(b1, gb, mask=gb.train_mask)
    g2 = copy.copy(gb)
    y = gb.y.clone()
    none = ~(gb.room_mask | gb.object_mask)
    y[none] = 999
    g2.y = y
    s2 = phase_a(b2, g2, mask=gb.train_mask)
    assert torch.equal(s1.grads, s2.grads)
    assert b2.native().read_state()[1] == 0


def test_row_in_both_heads_gets_both_contributions():
    gb = htree_batch("GraphSAGE", seed=5)
    gb.object_mask = gb.object_mask | gb.room_mask  # room rows also in the object head (labels < 15 suit both)
    a, b = twin_nets("GraphSAGE", True, dropout=0.25)
    check_against_autograd(a, b, gb, gb.train_mask)


@pytest.mark.parametrize("block", ["GraphSAGE", "GAT"])
def test_two_node_graphs(block):
    rng = np.random.Generator(np.random.PCG64(8))
    gb = collate_homogeneous([workloads.stanford_like_graph(rng, n_nodes=2) for _ in range(3)])
    gb.train_mask = torch.ones(gb.y.numel(), dtype=torch.bool)
    gb = gb.to(DEV)
    a, b = twin_nets(block)
    check_against_autograd(a, b, gb, gb.train_mask)


def test_ignored_label_rows_do_not_count():
    gb = stanford_batch("GraphSAGE", seed=13)
    ign = 3
    assert int(((gb.y == ign) & gb.train_mask).sum()) > 0
    a, b = twin_nets("GraphSAGE")
    step = check_against_autograd(a, b, gb, gb.train_mask & (gb.y != ign), ignored_label=ign)
    # the step was given train_mask itself: the ignored rows fell out of the count on the device
    assert float(step.grads[b.native().n_active + 1]) == float((gb.train_mask & (gb.y != ign)).sum())


def test_out_of_range_label_sets_status_bit():
    gb = stanford_batch("GraphSAGE")
    _, b = twin_nets("GraphSAGE")
    y = gb.y.clone()
    r = int(torch.nonzero(gb.train_mask & gb.room_mask)[0])
    y[r] = OUT["room"]  # valid object class, out of range for the room head
    step = b.semisupervised_step(lr=LR, use_graph=False)
    step(gb, labels=y)
    torch.cuda.synchronize()
    assert b.native().read_state()[1] & 2
    with pytest.raises(_lib.HydraMPError):
        step.loss()


def oracle_check(kw, gb, cnt_step=1):
    torch.manual_seed(4)
    ora = omodels.HomogeneousNetwork(**kw)
    with torch.no_grad():
        for name, p in ora.named_parameters():
            if name.endswith("bias"):
                p.add_(torch.randn_like(p) * 0.2)
    net = HomogeneousNetwork(**kw)
    net.load_state_dict(ora.state_dict(), strict=True)
    net = net.to(DEV)
    lib = _lib.require_device()

    def replay(x, p, training, tag):
        if not training or p == 0:
            return x
        layer = int(tag[1:].split(".", 1)[0])
        n, f = x.shape
        m = torch.zeros(max(n * f, 1), dtype=torch.uint8, device=DEV)
        if n * f:
            _lib.check(lib.hmp_dropout_mask(net._seed, cnt_step, net._drop_stream(layer), p, n, f, m.data_ptr(), _lib.stream_ptr()))
        return x * m[: n * f].view(n, f).cpu().to(x.dtype) / (1.0 - p)

    o64 = copy.deepcopy(ora).double().train()
    o64.dropout_fn = replay
    b64 = gb.to("cpu")
    b64.x = b64.x.double()
    if hasattr(b64, "edge_attr"):
        b64.edge_attr = b64.edge_attr.double()
    rm = b64.room_mask
    loss = o64.loss(o64(b64), (b64.y[rm], b64.y[~rm]), (b64.train_mask[rm], b64.train_mask[~rm]))
    loss.backward()
    step = phase_a(net, gb)
    assert abs(step.loss() - float(loss)) <= 1e-5 * max(1.0, abs(float(loss)))
    cnt = float(step.grads[net.native().n_active + 1])
    og = dict(o64.named_parameters())
    for name, p in net.named_parameters():
        if og[name].grad is None:
            continue
        g = grad_of(net, step, p).cpu().double() / cnt
        torch.testing.assert_close(g, og[name].grad, atol=2e-5, rtol=1e-4, msg=lambda m: f"{name}: {m}")
    assert {"post_mp_room.weight", "post_mp_object.bias"} <= set(og)


def test_gradient_matches_oracle_sage_odd_width():
    """F = 30 (not a multiple of 4), dropout 0.25 on the hidden layers and the tail, keep-masks replayed at draw number 1"""
    oracle_check(model_kw("GraphSAGE", dropout=0.25, hidden=30), stanford_batch("GraphSAGE", n=16, seed=17))


def test_gradient_matches_oracle_gat_768():
    """the Stanford GAT shape: 6 heads x 128 concat twice, F = 768 (attention dropout is not replayed: p = 0)"""
    kw = dict(input_dim=6, output_dim_dict=dict(OUT), conv_block="GAT", GAT_hidden_dims=[128, 128], GAT_heads=[6, 6],
              GAT_concats=[True, True], dropout=0.0)
    oracle_check(kw, stanford_batch("GAT", n=40, seed=19))


def reference_counts(net, data, mask):
    """SemiSupervisedTrainingJob.test's per-batch arithmetic (:198-257) on the autograd model"""
    net.eval()
    with torch.no_grad():
        pr, po = net(data)
    rm, om = data.room_mask, object_rows(net, data)
    out = []
    for pred, rows in ((pr, rm), (po, om)):
        m = mask[rows]
        out += [int((pred.argmax(dim=1)[m] == data.y[rows][m]).sum()), int(m.sum())]
    return out


@pytest.mark.parametrize("htree,block", [(False, "GraphSAGE"), (False, "GAT"), (True, "GraphSAGE"), (True, "GAT_edge")])
def test_count_correct_equals_reference_test(htree, block):
    gb = htree_batch(block) if htree else stanford_batch(block, n=30)
    a, _ = twin_nets(block, htree)
    step = a.semisupervised_step(lr=0.01, use_graph=False)
    for _ in range(3):  # away from the initial weights
        step(gb)
    for mask_name in ("train_mask", "val_mask", "test_mask"):
        want = reference_counts(a, gb, getattr(gb, mask_name))
        assert a.count_correct(gb, mask_name) == want
        acc = torch.zeros(4, dtype=torch.int64, device=DEV)
        a.count_correct(gb, mask_name, counts=acc)
        a.count_correct(gb, mask_name, counts=acc)
        assert acc.tolist() == [2 * v for v in want]


@pytest.mark.parametrize("block", ["GraphSAGE", "GAT"])
def test_two_runs_are_bitwise_equal(block):
    gb = stanford_batch(block, n=40)
    res = []
    for _ in range(2):
        _, b = twin_nets(block, seed=9)
        step = b.semisupervised_step(lr=LR, weight_decay=WD, use_graph=True)
        for _ in range(3):
            step(gb)
        torch.cuda.synchronize()
        res.append((step.flat.clone(), step.m.clone(), step.v.clone()))
    for x, y in zip(res[0], res[1]):
        assert torch.equal(x, y)


def test_refusals():
    gb = stanford_batch("GraphSAGE")
    room = HomogeneousNetwork(input_dim=6, output_dim=15, conv_block="GraphSAGE", hidden_dim=16, num_layers=2).to(DEV)
    with pytest.raises(_lib.HydraMPError):
        room.semisupervised_step(lr=1e-3)
    with pytest.raises(_lib.HydraMPError):
        room.count_correct(gb)
    _, b = twin_nets("GraphSAGE")
    with pytest.raises(NotImplementedError):
        b.train_step(lr=1e-3)
    step = b.semisupervised_step(lr=1e-3, use_graph=False)
    with pytest.raises(_lib.HydraMPError):
        step.run(None)


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_equal_single_rank_full_batch(tmp_path):
    """2 ranks sharing cuda:0 over gloo: phase A / flat all-reduce (heads included) / phase B == one rank, full batch"""
    world, port = 2, str(free_port())
    worker = os.path.join(HERE, "_two_head_homog_worker.py")
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(world), port, str(tmp_path / f"r{r}.pt")], env=env)
             for r in range(world)]
    for p in procs:
        try:
            assert p.wait(timeout=240) == 0
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    single = subprocess.run([sys.executable, worker, "0", "1", "0", str(tmp_path / "full.pt")], env=env, timeout=240)
    assert single.returncode == 0
    res = [torch.load(tmp_path / f"r{r}.pt", weights_only=True) for r in range(world)]
    full = torch.load(tmp_path / "full.pt", weights_only=True)
    assert torch.equal(res[0]["params"], res[1]["params"]) and res[0]["losses"] == res[1]["losses"]
    np.testing.assert_allclose(res[0]["losses"], full["losses"], rtol=2e-5, atol=2e-6)
    d = (res[0]["params"] - full["params"]).abs()
    assert float((d > 1e-5).double().mean()) < 0.01
    assert float(d.max()) <= 3 * LR * 2.1


def launches_of(net, step, gb, *args):
    step(gb, *args)  # warm (workspace, handle)
    torch.cuda.synchronize()
    h = net.native()._handle
    lib = net.native()._lib
    _lib.check(lib.hmp_net_profile(h, 1))
    step(gb, *args)
    torch.cuda.synchronize()
    ms = np.zeros(_lib.N_KCLASS, dtype=np.float32)
    n = np.zeros(_lib.N_KCLASS, dtype=np.int32)
    _lib.check(lib.hmp_net_profile_read(h, ms.ctypes.data_as(C.POINTER(C.c_float)), n.ctypes.data_as(C.POINTER(C.c_int32))))
    _lib.check(lib.hmp_net_profile(h, 0))
    return int(n.sum())


def test_launch_structure():
    """config-2-sized SAGE (hidden 64, 3 layers, B = 32): at most 2 launches more than the single-output step (the head kernel)"""
    gb = stanford_batch("GraphSAGE", n=32, seed=21)
    torch.manual_seed(0)
    kw = dict(input_dim=6, conv_block="GraphSAGE", hidden_dim=64, num_layers=3, dropout=0.25)
    two = HomogeneousNetwork(output_dim_dict=dict(OUT), **kw).to(DEV)
    one = HomogeneousNetwork(output_dim=35, **kw).to(DEV)
    n_two = launches_of(two, two.semisupervised_step(lr=LR, use_graph=False), gb)
    n_one = launches_of(one, one.train_step(lr=LR, ignored_label=-100, use_graph=False), gb, gb.y)
    assert n_two <= n_one + 2, (n_two, n_one)
