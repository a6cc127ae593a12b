"""Models whose GAT heads are wider than 256 channels, against ``oracle.models`` in float64.

* ``HomogeneousNeuralTreeNetwork(306, ...)`` with its default ``disable_initialization=False``: ``pre_mp`` is a one-head
  306 -> 306 GAT over ``init_edge_index``, applied to every node of the H-tree batch at its full 306 columns (about 70 % of the
  nodes have no incoming init edge and end up with the bias alone) -- logits, loss and every gradient, the four ``pre_mp.*``
  included; the fused step against ``loss.backward()`` + Adam on a twin; a stream batch against ``store.collate``; a training job
  against the hand-written loop.
* ``GAT_hidden_dims=[320]``: a wide concat layer (2 x 320) feeding a 640-wide input of the next layer, and a wide head mean whose
  320-wide state the tail and the two linear heads read.
* a heterogeneous GAT network with 320-wide heads on both node types.

Tolerance: 1e-5 (atol + rtol) against float64, as tests/test_gpu_htree.py and tests/test_gpu_gat.py; the fused step uses the twin-net
bounds of tests/test_gpu_semisupervised_homog.py; stream and job comparisons are exact."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_training_job as tj  # noqa: E402
from hydra_gnn_amd import workloads  # noqa: E402
from hydra_gnn_amd.data import collate_homogeneous  # noqa: E402
from hydra_gnn_amd.models import HomogeneousNetwork, HomogeneousNeuralTreeNetwork  # noqa: E402
from hydra_gnn_amd.store import GraphStore  # noqa: E402
from oracle import models as omodels  # noqa: E402
from test_gpu_gat import check_model, gat_pair  # noqa: E402
from test_gpu_homog_room_stream import homog_htree_graphs, where_labels  # noqa: E402
from test_gpu_htree import homogeneous_htree_batch  # noqa: E402
from test_gpu_semisupervised_homog import LR, WD, compare_params  # noqa: E402

ATOL, RTOL = 1e-5, 1e-5
DEV = "cuda:0"
IGNORED = 25
GAT3 = dict(GAT_hidden_dims=[16, 16], GAT_heads=[2, 2, 2], GAT_concats=[True, True, False])


def htree_kw(block, dropout=0.0):
    return dict(input_dim=306, output_dim=26, conv_block=block, hidden_dim=32, num_layers=3, dropout=dropout, **GAT3)


def grads_close(net, o64):
    og = dict(o64.named_parameters())
    for name, p in net.named_parameters():
        ref = og[name].grad
        if ref is None:
            assert p.grad is None, name
            continue
        assert p.grad is not None, name
        torch.testing.assert_close(p.grad.cpu().double(), ref, atol=ATOL, rtol=RTOL, msg=lambda m: f"{name}: {m}")


def room_parity(ora, net, batch, masked):
    """eval logits, loss and every gradient of a homogeneous room classifier against the float64 oracle"""
    net = net.to(DEV).eval()
    o64 = copy.deepcopy(ora).double().eval()
    b64 = batch.to("cpu")
    b64.x = b64.x.double()
    pred_ref = o64(b64)
    pred = net(batch.to(DEV))
    assert pred.shape == pred_ref.shape
    torch.testing.assert_close(pred.cpu().double(), pred_ref.detach(), atol=ATOL, rtol=RTOL)
    y = batch.y[batch.room_mask]
    yg = y.to(DEV)
    loss_ref = o64.loss(pred_ref, y, y != IGNORED) if masked else o64.loss(pred_ref, y)
    loss_ref.backward()
    loss = net.loss(pred, yg, yg != IGNORED) if masked else net.loss(pred, yg)
    torch.testing.assert_close(loss.cpu().double(), loss_ref.detach(), atol=ATOL, rtol=RTOL)
    loss.backward()
    grads_close(net, o64)
    return net, o64


@pytest.mark.parametrize("block", ["GraphSAGE", "GAT"])
def test_homogeneous_htree_parity_with_a_306_wide_pre_mp(block):
    torch.manual_seed(2)
    kw = htree_kw(block)
    ora = omodels.HomogeneousNeuralTreeNetwork(**kw)
    with torch.no_grad():
        ora.pre_mp.bias.uniform_(-0.2, 0.2)
    net = HomogeneousNeuralTreeNetwork(**kw)
    net.load_state_dict(ora.state_dict(), strict=True)
    batch = homogeneous_htree_batch(4, seed=41)
    assert batch.x.shape[1] == 306 and int(batch.room_mask.sum()) > 0
    fed = torch.bincount(batch.init_edge_index[1], minlength=batch.x.size(0)) > 0
    assert 0.5 < float((~fed).double().mean()) < 0.9  # bias-only rows
    net, o64 = room_parity(ora, net, batch, masked=True)
    for name in ("pre_mp.lin_src.weight", "pre_mp.att_src", "pre_mp.att_dst", "pre_mp.bias"):
        g = dict(net.named_parameters())[name].grad
        assert g is not None and float(g.abs().max()) > 0, name


def stanford_room_batch(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return collate_homogeneous([workloads.stanford_like_graph(rng, n_nodes=(2 if i == 0 else None)) for i in range(n)])


def randomise_biases(ora, scale=0.1):
    with torch.no_grad():
        for n_, p_ in ora.named_parameters():
            if n_.endswith(".bias"):
                p_.uniform_(-scale, scale)


def test_homogeneous_gat_320_wide_concat_then_640_wide_input():
    torch.manual_seed(1)
    kw = dict(input_dim=6, output_dim=15, conv_block="GAT", GAT_hidden_dims=[320], GAT_heads=[2, 2], GAT_concats=[True, False],
              dropout=0.0)
    ora = omodels.HomogeneousNetwork(**kw)
    randomise_biases(ora)
    net = HomogeneousNetwork(**kw)
    net.load_state_dict(ora.state_dict(), strict=True)
    assert tuple(ora.state_dict()["convs.1.lin_src.weight"].shape) == (30, 640)
    room_parity(ora, net, stanford_room_batch(6, 3), masked=False)


def test_homogeneous_two_heads_read_a_320_wide_head_mean():
    torch.manual_seed(3)
    kw = dict(input_dim=6, output_dim_dict={"room": 15, "object": 35}, conv_block="GAT", GAT_hidden_dims=[320], GAT_heads=[2],
              GAT_concats=[False], dropout=0.0)
    ora = omodels.HomogeneousNetwork(**kw)
    randomise_biases(ora)
    net = HomogeneousNetwork(**kw)
    net.load_state_dict(ora.state_dict(), strict=True)
    assert tuple(net.post_mp_room.weight.shape) == (15, 320)
    net = net.to(DEV).eval()
    batch = stanford_room_batch(6, 5)
    o64 = copy.deepcopy(ora).double().eval()
    b64 = batch.to("cpu")
    b64.x = b64.x.double()
    rr, ro = o64(b64)
    pr, po = net(batch.to(DEV))
    assert pr.shape == rr.shape and po.shape == ro.shape and po.shape[0] > 0
    torch.testing.assert_close(pr.detach().cpu().double(), rr.detach(), atol=ATOL, rtol=RTOL)
    torch.testing.assert_close(po.detach().cpu().double(), ro.detach(), atol=ATOL, rtol=RTOL)
    ((rr * rr).sum() / rr.shape[0] + ro.sum() / ro.shape[0]).backward()
    ((pr * pr).sum() / pr.shape[0] + po.sum() / po.shape[0]).backward()
    grads_close(net, o64)


def test_heterogeneous_gat_with_320_wide_heads():
    """hidden 320: every layer-0 destination is 2 x 320 wide, fed from 306-d objects and 6-d rooms; the last layer (26 wide, head
    mean) reads 640-wide inputs"""
    ora, net = gat_pair("GAT", [320], [2, 2], [True, False], seed=7)
    check_model(ora, net, workloads.mp3d_like_batch(3, seed=9))


def wide_twins(block, dropout=0.25, seed=0):
    torch.manual_seed(seed)
    a = HomogeneousNeuralTreeNetwork(**htree_kw(block, dropout))
    with torch.no_grad():
        a.pre_mp.bias.uniform_(-0.2, 0.2)
    b = copy.deepcopy(a)
    return a.to(DEV), b.to(DEV)


@pytest.mark.parametrize("block", ["GraphSAGE", "GAT"])
def test_fused_step_equals_autograd_loop_with_a_306_wide_pre_mp(block):
    """3 steps at dropout 0.25: net(data) -> loss -> backward -> torch.optim.Adam on a, train_step on its twin b (same seed, so the
    same keep-masks at the same step number)"""
    steps = 3
    gb = homogeneous_htree_batch(4, seed=43).to(DEV)
    labels = where_labels(gb)
    a, b = wide_twins(block)
    opt = torch.optim.Adam(a.parameters(), lr=LR, weight_decay=WD)
    tiny = {n: torch.zeros_like(p, dtype=torch.bool, device="cpu") for n, p in a.named_parameters()}
    a.train()
    losses_a = []
    for _ in range(steps):
        opt.zero_grad()
        y = gb.y[gb.room_mask]
        loss = a.loss(a(gb), y, y != IGNORED)
        loss.backward()
        for n, p in a.named_parameters():
            if p.grad is not None:
                tiny[n] |= (p.grad.abs() < 1e-5).cpu()
        opt.step()
        losses_a.append(float(loss))
    step = b.train_step(lr=LR, weight_decay=WD, ignored_label=IGNORED, use_graph=False, seed=b._seed)  # forward()'s masks
    losses_b = []
    for _ in range(steps):
        step(gb, labels)
        losses_b.append(step.loss())
    print(block, "losses", losses_a, losses_b)
    np.testing.assert_allclose(losses_b, losses_a, rtol=2e-5, atol=2e-6)
    compare_params(b, dict(a.named_parameters()), tiny, steps, f"{block}, 306-wide pre_mp")
    assert b.native().read_state() == (steps, 0)
    moved = (b.pre_mp.lin_src.weight.detach() - wide_twins(block)[1].pre_mp.lin_src.weight.detach()).abs().max()
    assert float(moved) > 0


def test_stream_batches_of_a_306_wide_pre_mp_model():
    """one step on a device-collated batch == one step on store.collate's batch, bit for bit; the counts and the predicted labels
    of the two agree"""
    gs = homog_htree_graphs(8, 4)
    a, b = wide_twins("GraphSAGE", seed=5)
    a, b = a.train(), b.train()
    store = GraphStore(gs, DEV)
    stream = store.stream(a, 4, label_type="node", ignored_label=IGNORED)
    sa = a.train_step(lr=LR, weight_decay=WD, ignored_label=IGNORED, use_graph=False)
    sb = b.train_step(lr=LR, weight_decay=WD, ignored_label=IGNORED, use_graph=False)
    ids = [0, 1, 2, 5]
    sa.run(stream.next(ids))
    gb = store.collate(ids)
    assert gb.x.shape[1] == 306
    sb(gb, where_labels(gb))
    la, lb = sa.loss(), sb.loss()
    assert la == lb and np.isfinite(la)
    assert torch.equal(sa.flat, sb.flat) and torch.equal(sa.m, sb.m) and torch.equal(sa.v, sb.v)
    assert a.native().read_state() == (1, 0) and b.native().read_state() == (1, 0)
    a.eval()
    ids = [4, 3, 6, 7]
    ref = store.collate(ids)
    h = stream.next(ids)
    got, want = a.count_correct_rooms(h), a.count_correct_rooms(ref)
    assert got == want and got[1] > 0
    lab_s = a.predict_labels(stream.next(ids)).clone()
    lab_c = a.predict_labels(ref)
    n = ref.x.size(0)
    assert torch.equal(lab_s[:n], lab_c[:n]) and int((lab_c[:n] >= 0).sum()) == int(ref.room_mask.sum())
    assert a.predict(ref).tolist() == lab_c[:n][ref.room_mask].tolist()


def test_room_job_on_306_wide_homogeneous_htrees_equals_the_hand_loop(tmp_path, monkeypatch):
    """BaseTrainingJob on ``homogeneous_htree`` data with the initialisation on (the constructor's default), 2 epochs"""
    name = "homog_htree_sage_init"
    case = ("homogeneous_htree", tj._homog_htree_graphs(80, 33), 306, 26, dict(conv_block="GraphSAGE", hidden_dim=32, num_layers=3))
    monkeypatch.setattr(tj, "room_case", lambda _name: case)
    train_kw = dict(decay_epochs=1, decay_rate=0.5, min_log_epoch=0)
    hand = tj.hand_room(name, 2, seed=17, **train_kw)
    job = tj.make_room_job(name)
    assert job._net.pre_mp is not None and job._net.input_dim == 306
    torch.manual_seed(17)
    out = job.train(str(tmp_path), dict(tj.OPT, num_epochs=2), **train_kw)
    tj.check_equal(out, hand)
    assert all(np.isfinite(out[2]["loss"])) and len(out[2]["loss"]) == 2
