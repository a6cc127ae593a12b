"""Fused step of the two-headed (room + object) task: ``HeterogeneousNetwork(output_dim_dict=...).semisupervised_step`` runs the
loop body of the reference's ``SemiSupervisedTrainingJob.train`` (semisupervised_training_job.py:117-147) natively, and
``count_correct`` the per-batch arithmetic of its ``test()`` (:198-257).  The step must equal the ``loss.backward()`` loop on the
same engine (same dropout masks), the oracle in float64, and the data-parallel protocol of the single-head step."""
import copy
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from hydra_gnn_amd import _lib, workloads  # noqa: E402
from hydra_gnn_amd.data import HeteroData, collate  # noqa: E402
from hydra_gnn_amd.models import HeterogeneousNetwork  # noqa: E402
from oracle import models as omodels  # noqa: E402

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
LR, WD = 0.002, 0.001
OUT = {"rooms": 26, "objects": 28}


def model_kw(block, dropout=0.25, hidden=32):
    kw = dict(input_dim_dict={"objects": 306, "rooms": 6}, output_dim_dict=dict(OUT), conv_block=block, hidden_dim=hidden,
              num_layers=3, dropout=dropout)
    if block != "GraphSAGE":
        kw.update(GAT_hidden_dims=[16, 16], GAT_heads=[2, 2, 2], GAT_concats=[True, True, False])
    if block == "GAT_edge":  # relative positions: the xyz columns move into edge_attr
        kw.update(input_dim_dict={"objects": 303, "rooms": 3})
    return kw


def twin_nets(block, dropout=0.25, seed=0, hidden=32):
    """two identical fresh models (same weights, same dropout seed, counters at 0)"""
    torch.manual_seed(seed)
    a = HeterogeneousNetwork(**model_kw(block, dropout, hidden))
    b = copy.deepcopy(a)
    return a.to(DEV), b.to(DEV)


def batch_of(block, n=8, seed=11):
    return workloads.semisupervised_batch(n, seed, relative_pos=block == "GAT_edge").to(DEV)


def targets(gb, mask="train_mask"):
    labels = (gb["rooms"].y, gb["objects"].y)
    masks = None if mask is None else (getattr(gb["rooms"], mask), getattr(gb["objects"], mask))
    return labels, masks


def flat_grad(net, p):
    nn_ = net.native()
    off = nn_.param_offsets[id(p)]
    return off, p.numel()


def compare_params(got, ref, tiny, steps, what):
    """the tolerance scheme of test_fused_train_step_matches_oracle_adam: Adam-ill-conditioned elements excluded and counted"""
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
    # (the GAT nets' attention / lin_edge gradients are small: about a fifth of their elements fall under 1e-5)
    assert n_tiny < 0.3 * n_all


@pytest.mark.parametrize("block", ["GraphSAGE", "GAT", "GAT_edge"])
def test_fused_step_equals_autograd_loop(block):
    """path A: net(batch) -> net.loss(pred, labels, masks) -> backward -> torch.optim.Adam; path B: semisupervised_step, eager and
    graph-replayed.  Dropout 0.25 (features, the tail, and GAT's attention coefficients): the masks are equal, so are the steps"""
    gb = batch_of(block)
    labels, masks = targets(gb)
    losses_a = []
    a, _ = twin_nets(block)
    opt = torch.optim.Adam(a.parameters(), lr=LR, weight_decay=WD)
    tiny = {n: torch.zeros_like(p, dtype=torch.bool, device="cpu") for n, p in a.named_parameters()}
    a.train()
    for _ in range(5):
        opt.zero_grad()
        loss = a.loss(a(gb), labels, masks)
        loss.backward()
        for n, p in a.named_parameters():
            if p.grad is not None:
                tiny[n] |= (p.grad.abs() < 1e-5).cpu()
        opt.step()
        losses_a.append(float(loss))
    ref = dict(a.named_parameters())
    for use_graph in (False, True):
        _, b = twin_nets(block)
        step = b.semisupervised_step(lr=LR, weight_decay=WD, use_graph=use_graph)
        losses_b = []
        for _ in range(5):
            step(gb, labels, masks)
            losses_b.append(step.loss())
        np.testing.assert_allclose(losses_b, losses_a, rtol=2e-5, atol=2e-6)
        compare_params(b, ref, tiny, 5, f"{block}, graph={use_graph}")
        assert b.native().read_state() == (5, 0)


def test_fused_step_matches_oracle():
    """SAGE two-head, dropout 0.25: 3 fused steps == oracle.models.HeterogeneousNetwork (float64) + torch.optim.Adam, the keep-masks
    (hidden layers and the tail) replayed through hmp_dropout_mask at the step number"""
    torch.manual_seed(4)
    kw = model_kw("GraphSAGE", 0.25, 64)
    ora = omodels.HeterogeneousNetwork(**kw)
    net = HeterogeneousNetwork(**kw)
    net.load_state_dict(ora.state_dict(), strict=True)
    net = net.to(DEV)
    gb = batch_of("GraphSAGE", 8, seed=5)
    labels, masks = targets(gb)
    lib = _lib.require_device()
    cur = {"step": 0}

    def replay(x, p, training, tag):
        if not training or p == 0:
            return x
        layer, t = tag[1:].split(".", 1)
        n, f = x.shape
        m = torch.zeros(max(n * f, 1), dtype=torch.uint8, device=DEV)
        if n * f:
            _lib.check(lib.hmp_dropout_mask(net._seed, cur["step"], net._drop_stream(int(layer), t), p, n, f, m.data_ptr(),
                                            _lib.stream_ptr()))
        return x * m[: n * f].view(n, f).cpu().to(x.dtype) / (1.0 - p)

    o64 = copy.deepcopy(ora).double().train()
    o64.dropout_fn = replay  # hidden layers and the two-headed tail (tag L{L-1}.<type>) draw through it
    b64 = gb.to("cpu")
    for t in b64.node_types:
        b64[t].x = b64[t].x.double()
    opt = torch.optim.Adam(o64.parameters(), lr=LR, weight_decay=WD)
    step = net.semisupervised_step(lr=LR, weight_decay=WD, use_graph=False)
    lab_c = tuple(y.cpu() for y in labels)
    msk_c = tuple(m.cpu() for m in masks)
    for k in range(1, 4):
        cur["step"] = k
        opt.zero_grad()
        loss = o64.loss(o64(b64), lab_c, msk_c)
        loss.backward()
        opt.step()
        step(gb, labels, masks)
        assert abs(step.loss() - float(loss)) <= 1e-5 * max(1.0, abs(float(loss)))
    ref = dict(o64.named_parameters())
    for name, p in net.named_parameters():
        d = (p.detach().cpu().double() - ref[name].detach()).abs()
        assert float((d > 5e-5).double().mean()) < 0.01, name
        assert float(d.max()) <= 3 * LR * 2.1, name


def one_step_grads(block, labels, masks, gb, **kw):
    """phase A only (force_collective without a process group: A, no-op all-reduce, B at lr 0): flat gradient sums + tail"""
    _, b = twin_nets(block)
    step = b.semisupervised_step(lr=0.0, use_graph=False, force_collective=True, **kw)
    step(gb, labels, masks)
    torch.cuda.synchronize()
    return b, step


def test_all_false_mask_drops_that_head():
    block = "GraphSAGE"
    gb = batch_of(block)
    labels, masks = targets(gb)
    masks = (masks[0], torch.zeros_like(masks[1]))
    a, _ = twin_nets(block)
    a.train()
    pr, _po = a(gb)
    loss = a.loss(pr, labels[0], masks[0])  # rooms only: mean CE over the room mask
    loss.backward()
    b, step = one_step_grads(block, labels, masks, gb)
    na = b.native().n_active
    count = float(step.grads[na + 1])
    assert count == float(masks[0].sum())
    assert abs(step.loss() - float(loss)) <= 2e-5 * max(1.0, abs(float(loss)))
    for p_ref, p in zip(a.parameters(), b.parameters()):
        off, n = flat_grad(b, p)
        if p_ref.grad is None:
            continue
        g = step.grads[off:off + n].view(p.shape) / count
        torch.testing.assert_close(g, p_ref.grad, atol=1e-6, rtol=1e-4)


def test_out_of_range_label_sets_status_bit():
    block = "GraphSAGE"
    gb = batch_of(block)
    labels, masks = targets(gb)
    yo = labels[1].clone()
    i = int(torch.nonzero(masks[1])[0])
    yo[i] = 99
    b, step = one_step_grads(block, (labels[0], yo), masks, gb)  # a fresh net: nothing clears the status word
    assert b.native().read_state()[1] & 2
    with pytest.raises(_lib.HydraMPError):
        step.loss()


@pytest.mark.parametrize("block", ["GraphSAGE", "GAT"])
def test_ignored_label_rows_do_not_count(block):
    gb = batch_of(block)
    labels, masks = targets(gb)
    yr = labels[0].clone()
    yr[::3] = -100
    a, _ = twin_nets(block)
    a.train()
    pr, po = a(gb)
    sel_r = masks[0] & (yr != -100)
    lsum = F.cross_entropy(pr[sel_r], yr[sel_r], reduction="sum") + F.cross_entropy(po[masks[1]], labels[1][masks[1]], reduction="sum")
    count = int(sel_r.sum()) + int(masks[1].sum())
    b, step = one_step_grads(block, (yr, labels[1]), masks, gb)
    na = b.native().n_active
    assert float(step.grads[na + 1]) == count
    assert abs(step.loss() - float(lsum) / count) <= 2e-5 * max(1.0, float(lsum) / count)


def reference_test_counts(net, gb, mask_name):
    """the reference's test() per batch, in torch on net(batch) in eval mode"""
    net.eval()
    with torch.no_grad():
        pred = [p.argmax(dim=1) for p in net(gb)]
    labels = (gb["rooms"].y, gb["objects"].y)
    masks = (getattr(gb["rooms"], mask_name), getattr(gb["objects"], mask_name))
    out = []
    for p, l, m in zip(pred, labels, masks):
        out += [int(p[m].eq(l[m]).sum()), int(torch.numel(l[m]))]
    return out


@pytest.mark.parametrize("block", ["GraphSAGE", "GAT"])
def test_count_correct_matches_reference_test(block):
    gb = batch_of(block)
    a, b = twin_nets(block)
    if block == "GraphSAGE":
        # every room logit negative: ReLU makes the whole row 0 and the argmax is the first index (torch's tie rule)
        with torch.no_grad():
            for name, p in b.named_parameters():
                if name.startswith(f"convs.{b.num_layers - 1}.") and name.endswith("rooms.lin_l.bias"):
                    p.add_(-1e3)
    for net in (a, b):
        for mask_name in ("train_mask", "val_mask", "test_mask"):
            want = reference_test_counts(net, gb, mask_name)
            labels, masks = targets(gb, mask_name)
            assert net.count_correct(gb, labels, masks) == want, (block, mask_name)
            acc = torch.zeros(4, dtype=torch.int64, device=DEV)
            net.count_correct(gb, labels, masks, counts=acc)
            net.count_correct(gb, labels, masks, counts=acc)
            assert acc.tolist() == [2 * v for v in want]
    if block == "GraphSAGE":
        b.eval()
        with torch.no_grad():
            pr, _ = b(gb)
        assert bool((pr == 0).all())  # the tie case really was exercised
        assert reference_test_counts(b, gb, "train_mask")[0] == int((gb["rooms"].y[gb["rooms"].train_mask] == 0).sum())


def tiny_graph(rng, n_rooms, n_obj, n_obj_classes):
    """a hand-sized scene graph of the MP3D shape: an object ring, a room chain, object i in room i % n_rooms"""
    ring = np.stack([np.arange(n_obj), (np.arange(n_obj) + 1) % n_obj])
    chain = np.stack([np.arange(n_rooms - 1), np.arange(1, n_rooms)])
    ro = np.stack([np.arange(n_obj) % n_rooms, np.arange(n_obj)])
    both = lambda e: torch.from_numpy(np.concatenate([e, e[::-1]], 1).astype(np.int64))
    g = HeteroData()
    for t, n, d, c in (("objects", n_obj, 306, n_obj_classes), ("rooms", n_rooms, 6, 5)):
        g[t].x = torch.from_numpy(rng.normal(0.0, 0.5, size=(n, d)).astype(np.float32))
        g[t].pos = g[t].x[:, :3].clone()
        g[t].y = torch.from_numpy(rng.integers(0, c, size=n).astype(np.int64))
    g["objects", "objects_to_objects", "objects"].edge_index = both(ring)
    g["rooms", "rooms_to_rooms", "rooms"].edge_index = both(chain)
    g["objects", "objects_to_rooms", "rooms"].edge_index = torch.from_numpy(ro[::-1].copy().astype(np.int64))
    g["rooms", "rooms_to_objects", "objects"].edge_index = torch.from_numpy(ro.astype(np.int64))
    return g


def test_seventy_object_classes():
    """70 object classes on the UNPOOLED two-head tail: a second quad per lane (16 lanes x 4) and a ragged last quad in its CE
    and its argmax; 3 graphs of <= 6 rooms and <= 12 objects.  One fused step == the autograd loop (loss and gradient sums at the
    tolerances of the tests above), count_correct == numpy's first-maximum argmax, and rows whose logits all tie predict class 0."""
    rng = np.random.Generator(np.random.PCG64(70))
    gb = collate([tiny_graph(rng, r, o, 70) for r, o in ((2, 5), (6, 12), (4, 9))])
    for t in ("rooms", "objects"):
        gb[t].train_mask = torch.from_numpy(rng.random(int(gb[t].y.numel())) < 0.7)
    gb = gb.to(DEV)
    gb["objects"].y[::4] = 0  # class 0 is labelled: the all-tied prediction below has rows to be right about
    labels, masks = targets(gb)
    torch.manual_seed(70)
    kw = dict(model_kw("GraphSAGE", 0.25, 16), output_dim_dict={"rooms": 5, "objects": 70})
    a = HeterogeneousNetwork(**kw)
    b, c = copy.deepcopy(a).to(DEV), copy.deepcopy(a).to(DEV)
    a = a.to(DEV)

    a.train()
    loss = a.loss(a(gb), labels, masks)
    loss.backward()
    step = b.semisupervised_step(lr=0.0, use_graph=False, force_collective=True)
    step(gb, labels, masks)
    torch.cuda.synchronize()
    count = float(step.grads[b.native().n_active + 1])
    assert count == float(masks[0].sum() + masks[1].sum())
    np.testing.assert_allclose(step.loss(), float(loss), rtol=2e-5, atol=2e-6)
    assert b.native().read_state()[1] == 0
    for p_ref, p in zip(a.parameters(), b.parameters()):
        if p_ref.grad is None:
            continue
        off, n = flat_grad(b, p)
        torch.testing.assert_close(step.grads[off:off + n].view(p.shape) / count, p_ref.grad, atol=1e-6, rtol=1e-4)

    with torch.no_grad():  # every object logit negative: ReLU makes the whole row 0
        for name, p in c.named_parameters():
            if name.startswith(f"convs.{c.num_layers - 1}.") and name.endswith("objects.lin_l.bias"):
                p.add_(-1e3)
    for net in (a, c):
        net.eval()
        with torch.no_grad():
            pred = [np.argmax(p.cpu().numpy(), axis=1) for p in net(gb)]  # numpy: the first maximum
        want = []
        for p, l, m in zip(pred, labels, masks):
            l, m = l.cpu().numpy(), m.cpu().numpy()
            want += [int((p[m] == l[m]).sum()), int(m.sum())]
        assert net.count_correct(gb, labels, masks) == want
    with torch.no_grad():
        po = c(gb)[1]
    assert po.shape[1] == 70 and bool((po == 0).all())  # the tie case really was exercised
    assert want[2] == int((labels[1][masks[1]] == 0).sum()) > 0


@pytest.mark.parametrize("width", [3, 130, 256, 260])
def test_object_head_widths_against_the_oracle(width):
    """Object-head widths around the tail's dispatch: 3 (one ragged quad), 130 and 256 (the last aggregation's fused ce_tail epilogue
    above 70 classes and at its widest, a padded width of 256), 260 (past it: the stand-alone tail, more than four quads per lane).
    Phase A of one fused step (SAGE two-head, dropout 0.25 on the hidden layers and the tail) against oracle.models in float64 with
    the keep-masks replayed: the loss at test_fused_step_matches_oracle's tolerance, the gradient sums / count at the tolerance of
    the autograd comparisons above."""
    rng = np.random.Generator(np.random.PCG64(width))
    gb = collate([tiny_graph(rng, r, o, width) for r, o in ((2, 5), (6, 12), (4, 9))])
    for t in ("rooms", "objects"):
        gb[t].train_mask = torch.from_numpy(rng.random(int(gb[t].y.numel())) < 0.7)
    gb = gb.to(DEV)
    labels, masks = targets(gb)
    torch.manual_seed(width)
    kw = dict(model_kw("GraphSAGE", 0.25, 16), output_dim_dict={"rooms": 5, "objects": width})
    ora = omodels.HeterogeneousNetwork(**kw)
    net = HeterogeneousNetwork(**kw)
    net.load_state_dict(ora.state_dict(), strict=True)
    net = net.to(DEV)
    lib = _lib.require_device()

    def replay(x, p, training, tag):
        if not training or p == 0:
            return x
        layer, t = tag[1:].split(".", 1)
        n, f = x.shape
        m = torch.zeros(max(n * f, 1), dtype=torch.uint8, device=DEV)
        if n * f:
            _lib.check(lib.hmp_dropout_mask(net._seed, 1, net._drop_stream(int(layer), t), p, n, f, m.data_ptr(), _lib.stream_ptr()))
        return x * m[: n * f].view(n, f).cpu().to(x.dtype) / (1.0 - p)

    o64 = copy.deepcopy(ora).double().train()
    o64.dropout_fn = replay
    b64 = gb.to("cpu")
    for t in b64.node_types:
        b64[t].x = b64[t].x.double()
    loss = o64.loss(o64(b64), tuple(y.cpu() for y in labels), tuple(m.cpu() for m in masks))
    loss.backward()

    step = net.semisupervised_step(lr=0.0, use_graph=False, force_collective=True)
    step(gb, labels, masks)
    torch.cuda.synchronize()
    count = float(step.grads[net.native().n_active + 1])
    assert count == float(masks[0].sum() + masks[1].sum())
    assert net.native().read_state()[1] == 0
    assert abs(step.loss() - float(loss)) <= 1e-5 * max(1.0, abs(float(loss)))
    ref = dict(o64.named_parameters())
    for name, p in net.named_parameters():
        if ref[name].grad is None:
            continue
        off, n = flat_grad(net, p)
        got = (step.grads[off:off + n].view(p.shape) / count).cpu().double()
        torch.testing.assert_close(got, ref[name].grad, atol=1e-6, rtol=1e-4, msg=lambda m: f"{name} (width {width}): {m}")


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_equal_single_rank_full_batch(tmp_path):
    """2 ranks sharing cuda:0 over gloo: phase A / flat all-reduce / phase B of the two-head step == one rank, full batch"""
    world, port = 2, str(free_port())
    worker = os.path.join(HERE, "_two_head_worker.py")
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
    # Adam amplifies 1e-7 gradient differences where |g| ~ eps (test_gpu_multirank.py): the bulk within 1e-5, nothing beyond the travel
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
    ms = (torch.zeros(_lib.N_KCLASS, dtype=torch.float32)).numpy()
    n = np.zeros(_lib.N_KCLASS, dtype=np.int32)
    import ctypes as C

    _lib.check(lib.hmp_net_profile_read(h, ms.ctypes.data_as(C.POINTER(C.c_float)), n.ctypes.data_as(C.POINTER(C.c_int32))))
    _lib.check(lib.hmp_net_profile(h, 0))
    return int(n.sum())


@pytest.mark.parametrize("block,extra", [("GraphSAGE", 0), ("GAT", 1)])
def test_launch_structure(block, extra):
    """config-2-shaped (B = 32, hidden 64, 3 layers): the two-head step issues no more launches than the single-output step of the
    same architecture (SAGE: tail + CE in the last epilogue), at most one more on GAT (one stand-alone tail launch)"""
    kw = model_kw(block, 0.25, 64)
    if block == "GAT":
        kw.update(GAT_hidden_dims=[64, 64], GAT_heads=[2, 2, 2])
    gb = batch_of(block, 32, seed=21)
    torch.manual_seed(0)
    two = HeterogeneousNetwork(**kw).to(DEV)
    kw1 = dict(kw)
    kw1.pop("output_dim_dict")
    one = HeterogeneousNetwork(output_dim=26, **kw1).to(DEV)
    labels, masks = targets(gb)
    n_two = launches_of(two, two.semisupervised_step(lr=LR, use_graph=False), gb, labels, masks)
    n_one = launches_of(one, one.train_step(lr=LR, ignored_label=25, use_graph=False), gb, gb["rooms"].y)
    assert n_two <= n_one + extra, (n_two, n_one)
