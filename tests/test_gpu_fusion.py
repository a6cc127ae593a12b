"""Small-batch fusions (row-local GEMMs and the masked cross entropy riding in the aggregation kernels, Adam riding in the
gradient un-pack) against the stand-alone kernels and against the oracle.

HMP_FUSE=0 / 1 pins the executor to the stand-alone / fused launch sequence (read when the native net is created);
unset = automatic (fused up to 65536 nodes per batch at hidden 64, 16384 for wider layers).  Both sequences must satisfy the oracle tolerance, and they must
agree with each other far inside it (they differ only in fp32 summation order of the projections).
"""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hydra_gnn_amd import workloads  # noqa: E402
from hydra_gnn_amd.models import HeterogeneousNetwork, HeterogeneousNeuralTreeNetwork  # noqa: E402
from oracle import models as omodels  # noqa: E402

ATOL, RTOL = 1e-5, 1e-5
DEV = "cuda:0"
HT_DIMS = {"object": 306, "room": 6, "object-room": 6, "room-room": 6, "object_virtual": 306, "room_virtual": 6}


class fuse_env:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("HMP_FUSE")
        if self.value is None:
            os.environ.pop("HMP_FUSE", None)
        else:
            os.environ["HMP_FUSE"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("HMP_FUSE", None)
        else:
            os.environ["HMP_FUSE"] = self.old


def build(kw, cls, ocls, sd=None, seed=0):
    torch.manual_seed(seed)
    ora = ocls(**kw)
    if sd is not None:
        ora.load_state_dict(sd)
    net = cls(**kw)
    net.load_state_dict(ora.state_dict(), strict=True)
    return ora, net.to(DEV)


def run_fwd_bwd(net, batch, label_type, train=False):
    net.train(train)
    gb = batch.to(DEV)
    pred = net(gb)
    y = gb[label_type].y
    loss = net.loss(pred, y, y != 25)
    loss.backward()
    grads = {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in net.named_parameters()}
    return pred.detach().clone(), loss.detach().clone(), grads


SAGE_KW = dict(input_dim_dict={"objects": 306, "rooms": 6}, output_dim=26, conv_block="GraphSAGE", hidden_dim=64, num_layers=3,
               dropout=0.0)


@pytest.mark.parametrize("hidden,layers,dropout", [(64, 3, 0.0), (128, 4, 0.0), (256, 3, 0.0), (64, 3, 0.25), (48, 3, 0.0), (40, 3, 0.0)])
def test_fused_and_standalone_sequences_agree(hidden, layers, dropout):
    """(48: K % 16 == 0 -> fused; 40: not a multiple of 16 -> the forward projection silently stays stand-alone)"""
    kw = dict(SAGE_KW, hidden_dim=hidden, num_layers=layers, dropout=dropout)
    batch = workloads.config2_batch(8)
    res = {}
    for mode in ("0", "1"):
        with fuse_env(mode):
            _, net = build(kw, HeterogeneousNetwork, omodels.HeterogeneousNetwork)
            res[mode] = run_fwd_bwd(net, batch, "rooms", train=dropout > 0)
    p0, l0, g0 = res["0"]
    p1, l1, g1 = res["1"]
    torch.testing.assert_close(p1, p0, atol=2e-6, rtol=2e-6)
    torch.testing.assert_close(l1, l0, atol=2e-6, rtol=2e-6)
    for k in g0:
        assert (g0[k] is None) == (g1[k] is None)
        if g0[k] is not None:
            torch.testing.assert_close(g1[k], g0[k], atol=2e-6, rtol=2e-5, msg=lambda m: f"{k}: {m}")


@pytest.mark.parametrize("mode", ["0", "1"])
def test_both_sequences_match_the_oracle(mode):
    batch = workloads.config2_batch(8)
    with fuse_env(mode):
        ora, net = build(SAGE_KW, HeterogeneousNetwork, omodels.HeterogeneousNetwork)
        pred, loss, grads = run_fwd_bwd(net, batch, "rooms")
    o64 = copy.deepcopy(ora).double()
    b64 = batch.to("cpu")
    for t in b64.node_types:
        b64[t].x = b64[t].x.double()
    pred_ref = o64(b64)
    y = batch["rooms"].y
    loss_ref = o64.loss(pred_ref, y, y != 25)
    loss_ref.backward()
    torch.testing.assert_close(pred.cpu().double(), pred_ref.detach(), atol=ATOL, rtol=RTOL)
    torch.testing.assert_close(loss.cpu().double(), loss_ref.detach(), atol=ATOL, rtol=RTOL)
    for name, p in o64.named_parameters():
        if p.grad is not None:
            torch.testing.assert_close(grads[name].cpu().double(), p.grad, atol=ATOL, rtol=RTOL, msg=lambda m: f"{name}: {m}")


@pytest.mark.parametrize("use_graph", [False, True])
def test_fused_step_equals_two_phase_step(use_graph):
    """cross entropy in the last aggregation + Adam in the gradient un-pack == loss kernel + Adam kernel (5 steps, dropout on:
    both draw the same dropout masks)"""
    kw = dict(SAGE_KW, dropout=0.25)
    batch = workloads.config2_batch(8).to(DEV)
    y = batch["rooms"].y
    out = {}
    for mode in ("0", "1"):
        with fuse_env(mode):
            _, net = build(kw, HeterogeneousNetwork, omodels.HeterogeneousNetwork)
            net.train()
            step = net.train_step(lr=0.002, weight_decay=0.001, ignored_label=25, seed=99, use_graph=use_graph)
            losses = []
            for _ in range(5):
                step(batch, y)
                losses.append(step.loss())
            st, status = net.native().read_state()
            assert st == 5 and status == 0
            out[mode] = (losses, {k: p.detach().clone() for k, p in net.named_parameters()})
    np.testing.assert_allclose(out["1"][0], out["0"][0], rtol=1e-5, atol=1e-6)
    for k, p0 in out["0"][1].items():
        # Adam divides by |g|: where |g| ~ eps a 1e-7 difference in g moves the parameter by a fraction of lr (the bound)
        d = (out["1"][1][k] - p0).abs()
        assert float(d.max()) <= 5 * 0.002 * 2.1, k
        assert float((d > 2e-5).double().mean()) < 0.01, k


def test_fused_cross_entropy_edge_cases():
    """all labels ignored in one batch, an out-of-range label flagged in the status word (not a crash)"""
    with fuse_env("1"):
        _, net = build(SAGE_KW, HeterogeneousNetwork, omodels.HeterogeneousNetwork)
        batch = workloads.config2_batch(4).to(DEV)
        step = net.train_step(lr=0.002, weight_decay=0.0, ignored_label=25, use_graph=False)
        before = {k: p.detach().clone() for k, p in net.named_parameters()}
        y = torch.full_like(batch["rooms"].y, 25)
        step(batch, y)
        assert step.loss() == 0.0
        for k, p in net.named_parameters():  # zero gradient, no weight decay: Adam leaves the weights alone
            assert torch.equal(p.detach(), before[k]), k
        y2 = batch["rooms"].y.clone()
        y2[0] = 99
        step(batch, y2)
        _, status = net.native().read_state()
        assert status & 2


def test_htree_sequences_agree_and_pool_path_finalises_loss():
    kw = dict(input_dim_dict=HT_DIMS, output_dim=26, conv_block="GraphSAGE", hidden_dim=128, num_layers=4,
              disable_initialization=True, dropout=0.0)
    batch = workloads.htree_batch(4, seed=5)
    res, steps = {}, {}
    for mode in ("0", "1"):
        with fuse_env(mode):
            _, net = build(kw, HeterogeneousNeuralTreeNetwork, omodels.HeterogeneousNeuralTreeNetwork)
            res[mode] = run_fwd_bwd(net, batch, "room_virtual")
            gb = batch.to(DEV)
            step = net.train_step(lr=0.001, weight_decay=0.001, ignored_label=25, use_graph=False)
            ls = []
            for _ in range(3):
                step(gb, gb["room_virtual"].y)
                ls.append(step.loss())
            steps[mode] = ls
    torch.testing.assert_close(res["1"][0], res["0"][0], atol=2e-6, rtol=2e-6)
    for k, g in res["0"][2].items():
        if g is not None:
            torch.testing.assert_close(res["1"][2][k], g, atol=2e-6, rtol=2e-5, msg=lambda m: f"{k}: {m}")
    np.testing.assert_allclose(steps["1"], steps["0"], rtol=1e-5, atol=1e-6)
    assert steps["1"][-1] < steps["1"][0]


@pytest.mark.parametrize("var,kw_over", [("HMP_FRONT", {}), ("HMP_TN", {}), ("HMP_FRONT", {"hidden_dim": 128, "num_layers": 4})])
def test_front_kernel_and_direct_weight_gradient_agree_with_separate_launches(monkeypatch, var, kw_over):
    """HMP_FRONT=0: pack, layer-0 projection and plan as separate launches; HMP_TN=0: LDS-staged split-K weight gradients"""
    kw = dict(SAGE_KW, **kw_over)
    batch = workloads.config2_batch(8)
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv(var, mode)
        with fuse_env("1"):
            _, net = build(kw, HeterogeneousNetwork, omodels.HeterogeneousNetwork)
            res[mode] = run_fwd_bwd(net, batch, "rooms")
            step = net.train_step(lr=0.002, weight_decay=0.001, ignored_label=25, use_graph=False)
            gb = batch.to(DEV)
            for _ in range(3):
                step(gb, gb["rooms"].y)
            res[mode] += (step.loss(), {k: p.detach().clone() for k, p in net.named_parameters()})
    monkeypatch.delenv(var)
    torch.testing.assert_close(res["1"][0], res["0"][0], atol=2e-6, rtol=2e-6)
    for k, g in res["0"][2].items():
        if g is not None:
            torch.testing.assert_close(res["1"][2][k], g, atol=2e-6, rtol=2e-5, msg=lambda m: f"{k}: {m}")
    assert abs(res["1"][3] - res["0"][3]) < 1e-5
    for k, p0 in res["0"][4].items():
        d = (res["1"][4][k] - p0).abs()
        assert float(d.max()) <= 3 * 0.002 * 2.1, k
        assert float((d > 2e-5).double().mean()) < 0.01, k


def test_front_kernel_odd_shapes(monkeypatch):
    """rooms-only tiles, a node type with K = 6 (one ragged stage), hidden 40 (segments that straddle 64-column tiles); the weight
    gradients on the register-direct TN kernel (HMP_TN unset) and on the LDS-staged split-K kernel (HMP_TN=0), both against the
    oracle, and bitwise different from each other (the staged kernel really ran)"""
    kw = dict(SAGE_KW, hidden_dim=40)
    batch = workloads.config2_batch(3)
    weight_grads = {}
    for tn in (None, "0"):
        if tn is None:
            monkeypatch.delenv("HMP_TN", raising=False)
        else:
            monkeypatch.setenv("HMP_TN", tn)
        with fuse_env("1"):
            ora, net = build(kw, HeterogeneousNetwork, omodels.HeterogeneousNetwork)
            pred, loss, grads = run_fwd_bwd(net, batch, "rooms")
        o64 = copy.deepcopy(ora).double()
        b64 = batch.to("cpu")
        for t in b64.node_types:
            b64[t].x = b64[t].x.double()
        pred_ref = o64(b64)
        y = batch["rooms"].y
        o64.loss(pred_ref, y, y != 25).backward()
        torch.testing.assert_close(pred.cpu().double(), pred_ref.detach(), atol=ATOL, rtol=RTOL)
        for name, p in o64.named_parameters():
            if p.grad is not None:
                torch.testing.assert_close(grads[name].cpu().double(), p.grad, atol=ATOL, rtol=RTOL, msg=lambda m: f"{tn} {name}: {m}")
        weight_grads[tn] = {k: g for k, g in grads.items() if g is not None and g.dim() == 2}
    monkeypatch.delenv("HMP_TN", raising=False)
    assert any(not torch.equal(g, weight_grads["0"][k]) for k, g in weight_grads[None].items()), "HMP_TN=0 changed no weight gradient"


def test_bf16_compute_mode_on_a_large_graph():
    """precision='bf16' only touches GEMM calls with >= 1024 64x64 tiles: a 40k-object graph with hidden 256 takes the bf16 path for
    its projections; logits and loss stay within bf16 rounding of the fp32 engine, the fp32 mode is unchanged, small batches are
    bit-identical in both modes."""
    kw = dict(input_dim_dict={"objects": 256, "rooms": 256}, output_dim=26, conv_block="GraphSAGE", hidden_dim=256, num_layers=3, dropout=0.0)
    g = workloads.big_hetero_graph(n_obj=40000, n_rooms=400, seed=3).to(DEV)  # >= 32768 nodes: the 256x256-tile weight-gradient path + colsum kernel
    _, net = build(kw, HeterogeneousNetwork, omodels.HeterogeneousNetwork)
    net.eval()
    y = g["rooms"].y

    def fwd_bwd():
        for p in net.parameters():
            p.grad = None
        pred = net(g)
        net.loss(pred, y, y != 25).backward()
        return pred.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}

    ref, gref = fwd_bwd()
    net.native().set_compute("bf16")
    out, gout = fwd_bwd()
    assert not torch.equal(out, ref)  # the bf16 path really ran
    rel = float((out - ref).abs().max() / ref.abs().max())
    assert rel < 2e-2, rel
    for k, gr in gref.items():  # weights, root weights and biases (the ones-column path of the bf16 weight-gradient GEMM)
        # bf16 operand rounding (2^-9 per product) through 3 layers forward and backward, plus ReLU masks that flip where a
        # pre-activation is within that noise of zero: up to ~4 % in norm for the first layer's weights (measured 3.9 %)
        err = float((gout[k] - gr).norm() / (gr.norm() + 1e-20))
        assert err < 8e-2, (k, err)
        assert float((gout[k] - gr).abs().max() / (gr.abs().max() + 1e-20)) < 0.25, k
    # bf16 STORAGE of the projected rows / input gradients (on by default in this regime) against fp32 storage: same
    # computation, one more rounding to bf16 per stored element
    os.environ["HMP_Z16"] = "0"
    try:
        out32, g32 = fwd_bwd()
    finally:
        del os.environ["HMP_Z16"]
    assert not torch.equal(out32, out)  # the bf16-storage path really ran by default
    assert float((out32 - out).abs().max() / ref.abs().max()) < 2e-2
    for k, gr in g32.items():
        assert float((gout[k] - gr).norm() / (gr.norm() + 1e-20)) < 8e-2, k  # same budget as against fp32 compute (ReLU mask flips)
    small = workloads.config2_batch(2)
    _, net2 = build(SAGE_KW, HeterogeneousNetwork, omodels.HeterogeneousNetwork)
    net2.eval()
    a = net2(small.to(DEV)).detach().clone()
    net2.native().set_compute("bf16")
    assert torch.equal(net2(small.to(DEV)), a)


@pytest.mark.parametrize("n_obj,n_rooms", [(40000, 400), (140000, 4200)])
def test_bf16_mode_activation_storage_is_bit_identical(n_obj, n_rooms, monkeypatch):
    """(With every conv evaluated project-first, HMP_AGG_FIRST=0: an aggregate-first conv averages the STORED activations, so there
    the storage type is part of the result -- tests/test_gpu_config5.py holds that path to the bf16-storage contract instead.)
    bf16 compute mode, 256-wide hidden layers: the activations H of the hidden layers are written as bf16 by the aggregation
    and read as bf16 by the next projection, its weight gradient and the activation / dropout mask of its input gradient.
    Those GEMMs round H to bf16 on the way into LDS anyway and the dropout keep-bit is the sign of zero, so logits and every
    gradient must be BIT-identical to fp32-stored activations (HMP_H16=0), in training mode with dropout."""
    kw = dict(input_dim_dict={"objects": 256, "rooms": 256}, output_dim=26, conv_block="GraphSAGE", hidden_dim=256, num_layers=3, dropout=0.25)
    # 40 000 / 400: 128x128 GEMM tiles (a 400-row companion problem, < 2^17 nodes); 140 000 / 4 200: the 256x256 tiles of
    # config 5 for all three GEMM forms (every problem >= 4096 rows, weight gradients over >= 2^17 nodes)
    monkeypatch.setenv("HMP_AGG_FIRST", "0")
    g = workloads.big_hetero_graph(n_obj=n_obj, n_rooms=n_rooms, seed=9).to(DEV)
    _, net = build(kw, HeterogeneousNetwork, omodels.HeterogeneousNetwork)
    net.train()
    net.native().set_compute("bf16")
    y = g["rooms"].y

    def fwd_bwd():
        net._rng_step = 0  # same dropout masks in every run
        for p in net.parameters():
            p.grad = None
        pred = net(g)
        net.loss(pred, y, y != 25).backward()
        return pred.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}

    out, grads = fwd_bwd()
    os.environ["HMP_H16"] = "0"
    try:
        out32, g32 = fwd_bwd()
    finally:
        del os.environ["HMP_H16"]
    assert torch.equal(out, out32)
    assert set(grads) == set(g32)
    for k in grads:
        assert torch.equal(grads[k], g32[k]), k
    # same for the root block of dZ: by default the backward GEMMs read it straight from the bf16 output gradient
    # (GemmProblem::A2), with HMP_ROOTCOPY=1 the transposed aggregation copies it into dZ first -- the same bits either way
    os.environ["HMP_ROOTCOPY"] = "1"
    try:
        outc, gc = fwd_bwd()
    finally:
        del os.environ["HMP_ROOTCOPY"]
    assert torch.equal(out, outc)
    for k in grads:
        assert torch.equal(grads[k], gc[k]), k
    net.eval()  # and the dropout really acted (train != eval), i.e. the keep bits were read
    assert not torch.equal(net(g), out)


@pytest.mark.parametrize("n_obj,n_rooms,shuffle", [(40000, 400, False), (140000, 1400, False), (40000, 400, True)])
def test_lds_windowed_aggregation_against_plain_kernels(n_obj, n_rooms, shuffle, monkeypatch):
    """bf16 mode, 256-wide layers, >= 16384 rows: persistent workgroups keep a sliding ring of source rows in LDS and serve
    in-window neighbours from there (agg_fwd_win_kernel / agg_bwd_win_kernel); a row's out-of-window rows are requested first and
    added behind the in-window ones (round 3) -- another association of the same fp32 sum than the plain one-wave-per-row kernels'
    (HMP_AGG_WIN=0), but sums of <= 20 bf16 numbers of one layer's scale are EXACT in fp32, so logits and every gradient still
    come out with the same bits on these graphs: also when the numbering has no locality at all (object ids shuffled: nearly every
    neighbour is out of the window, several rounds of four per row) and in training mode with dropout.  (Should a new graph ever
    break the equality by a rounding, this comparison has to take a tolerance; the oracle comparison is tests/test_gpu_config5.py.)"""
    monkeypatch.setenv("HMP_BF16_ALL", "1")
    kw = dict(input_dim_dict={"objects": 256, "rooms": 256}, output_dim=26, conv_block="GraphSAGE", hidden_dim=256, num_layers=3, dropout=0.25)
    g = workloads.big_hetero_graph(n_obj=n_obj, n_rooms=n_rooms, seed=13)
    if shuffle:  # relabel the objects at random: destroys the locality the window relies on, not the graph
        perm = torch.randperm(n_obj, generator=torch.Generator().manual_seed(5))
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(n_obj)
        g["objects"].x = g["objects"].x[perm]
        oo = ("objects", "objects_to_objects", "objects")
        g[oo].edge_index = inv[g[oo].edge_index]
        o2r = ("objects", "objects_to_rooms", "rooms")
        ei = g[o2r].edge_index.clone(); ei[0] = inv[ei[0]]; g[o2r].edge_index = ei
        r2o = ("rooms", "rooms_to_objects", "objects")
        ei = g[r2o].edge_index.clone(); ei[1] = inv[ei[1]]; g[r2o].edge_index = ei
    g = g.to(DEV)
    _, net = build(kw, HeterogeneousNetwork, omodels.HeterogeneousNetwork)
    net.train()
    net.native().set_compute("bf16")
    y = g["rooms"].y

    def fwd_bwd():
        net._rng_step = 0
        for p in net.parameters():
            p.grad = None
        pred = net(g)
        net.loss(pred, y, y != 25).backward()
        return pred.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}

    monkeypatch.setenv("HMP_AGG_WIN", "0")
    ref, gref = fwd_bwd()
    assert net.native().read_state()[1] == 0
    monkeypatch.delenv("HMP_AGG_WIN")
    out, grads = fwd_bwd()
    assert torch.equal(out, ref)
    assert set(grads) == set(gref)
    for k in grads:
        assert torch.equal(grads[k], gref[k]), k
    assert net.native().read_state()[1] == 0


@pytest.mark.parametrize("hidden", [64, 256])
def test_large_launch_xcd_row_mapping_is_bit_identical(hidden, monkeypatch):
    """>= 65536 rows: the aggregation kernels hand every XCD one contiguous eighth of the rows (L2 locality).  Which block
    computes a row must not change the row: logits and every gradient are bit-identical to the plain block order, and the
    logits stay within tolerance of the float64 oracle (sums over 10^5 rows are compared at 1e-4)."""
    kw = dict(input_dim_dict={"objects": 64, "rooms": 64}, output_dim=26, conv_block="GraphSAGE", hidden_dim=hidden, num_layers=3, dropout=0.0)
    g = workloads.big_hetero_graph(n_obj=70001, n_rooms=701, deg=6, feat_dim=64, seed=5)
    ora, net = build(kw, HeterogeneousNetwork, omodels.HeterogeneousNetwork)
    net.eval()
    gd = g.to(DEV)
    y = gd["rooms"].y

    def fwd_bwd():
        for p in net.parameters():
            p.grad = None
        pred = net(gd)
        net.loss(pred, y, y != 25).backward()
        return pred.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}

    out, grads = fwd_bwd()
    for env in ({"HMP_AGG_XCD": "0"},):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out0, grads0 = fwd_bwd()
        for k in env:
            monkeypatch.delenv(k)
        assert torch.equal(out, out0), env
        for k in grads:
            assert torch.equal(grads[k], grads0[k]), (k, env)
    o64 = copy.deepcopy(ora).double().eval()
    b64 = g.to("cpu")
    for t in b64.node_types:
        b64[t].x = b64[t].x.double()
    with torch.no_grad():
        ref = o64(b64)
    torch.testing.assert_close(out.cpu().double(), ref, atol=1e-4, rtol=1e-4)


def test_bf16_mode_htree_many_edge_types():
    """bf16 compute mode with bf16-stored Z / G / dZ on the H-tree program (up to 6 incoming edge types per node type, LeafPool
    readout) at > 65 536 nodes: logits and gradients stay within bf16 rounding of the fp32 engine."""
    dims = {"object": 306, "room": 6, "object-room": 6, "room-room": 6, "object_virtual": 306, "room_virtual": 6}
    kw = dict(input_dim_dict=dims, output_dim=26, conv_block="GraphSAGE", hidden_dim=256, num_layers=3, disable_initialization=True,
              dropout=0.0)
    torch.manual_seed(3)
    net = HeterogeneousNeuralTreeNetwork(**kw).to(DEV).eval()
    g = workloads.htree_batch(96, seed=77).to(DEV)
    assert sum(int(g[t].num_nodes) for t in g.node_types) > 65536
    y = g["room_virtual"].y

    def fwd_bwd():
        for p in net.parameters():
            p.grad = None
        pred = net(g)
        net.loss(pred, y, y != 25).backward()
        return pred.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}

    ref, gref = fwd_bwd()
    net.native().set_compute("bf16")
    out, gout = fwd_bwd()
    assert not torch.equal(out, ref)
    assert float((out - ref).abs().max() / ref.abs().max()) < 3e-2
    for k, gr in gref.items():
        assert float((gout[k] - gr).norm() / (gr.norm() + 1e-20)) < 0.1, k


@pytest.mark.parametrize("tall,hidden", [("1", 64), ("0", 64), ("1", 48)])
def test_standalone_sequence_at_the_reference_batch_scale_matches_the_oracle(monkeypatch, tall, hidden):
    """config/mp3d/*.yaml train with batch_size 2048 (~190 000 nodes): far above the small-batch threshold, i.e. the stand-alone
    launch sequence (grouped fp32 MFMA GEMMs + one-row-group aggregation, hidden 64).  At 512 graphs (46 000 nodes, a size the
    float64 oracle holds) with that sequence pinned: logits, loss and every gradient at the north_star tolerance.  The weight
    gradients over the 45 000 objects run on the tall split-K kernel (HMP_GEMM_TALL=0: the 64x64-tile one)."""
    monkeypatch.setenv("HMP_FUSE", "0")
    monkeypatch.setenv("HMP_GEMM_TALL", tall)
    ora, net = build(dict(SAGE_KW, hidden_dim=hidden), HeterogeneousNetwork, omodels.HeterogeneousNetwork, seed=4)
    batch = workloads.config2_batch(512)
    o64 = copy.deepcopy(ora).double().eval()
    b64 = batch.to("cpu")
    for t in b64.node_types:
        b64[t].x = b64[t].x.double()
    y = batch["rooms"].y
    pred_ref = o64(b64)
    loss_ref = o64.loss(pred_ref, y, y != 25)
    loss_ref.backward()
    pred, loss, grads = run_fwd_bwd(net, batch, "rooms")
    torch.testing.assert_close(pred.cpu().double(), pred_ref.detach(), atol=ATOL, rtol=RTOL)
    torch.testing.assert_close(loss.cpu().double(), loss_ref.detach(), atol=ATOL, rtol=RTOL)
    for name, p in o64.named_parameters():
        if p.grad is not None:
            # sums over 46 000 nodes in fp32: 1e-5 relative + 1e-5 of the tensor's scale
            scale = max(float(p.grad.abs().max()), 1.0)
            torch.testing.assert_close(grads[name].cpu().double(), p.grad, atol=ATOL * scale, rtol=RTOL, msg=lambda m: f"{name}: {m}")


@pytest.mark.parametrize("kw_over,n_graphs", [({}, 32), ({}, 1), ({"hidden_dim": 128, "num_layers": 4}, 9), ({}, 300)])
def test_plan_from_graph_sorted_edge_lists_is_bit_identical(monkeypatch, kw_over, n_graphs):
    """collate() records where each graph's edges start (the per-edge-type ptr): the single-launch plan build then reads, per
    block of rows, only the edges of the graphs that own those rows (hmp_batch::d_edge_ptr).  HMP_PLAN_SLICED=0 reads the whole
    list per block as before: same CSR / CSC arrays, so predictions, gradients and optimiser steps are bit-identical."""
    kw = dict(SAGE_KW, **kw_over)
    batch = workloads.config2_batch(n_graphs)
    assert batch["objects", "objects_to_objects", "objects"].ptr.numel() == n_graphs + 1
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("HMP_PLAN_SLICED", mode)
        with fuse_env("1"):
            _, net = build(kw, HeterogeneousNetwork, omodels.HeterogeneousNetwork)
            res[mode] = run_fwd_bwd(net, batch, "rooms")
            assert net.native().read_state()[1] == 0
            step = net.train_step(lr=0.002, weight_decay=0.001, ignored_label=25, use_graph=False)
            gb = batch.to(DEV)
            for _ in range(3):
                step(gb, gb["rooms"].y)
            res[mode] += (step.loss(), {k: p.detach().clone() for k, p in net.named_parameters()})
            assert net.native().read_state()[1] == 0
    monkeypatch.delenv("HMP_PLAN_SLICED")
    assert torch.equal(res["1"][0], res["0"][0])
    for k, g in res["0"][2].items():
        if g is not None:
            assert torch.equal(res["1"][2][k], g), k
    assert res["1"][3] == res["0"][3]
    for k, p0 in res["0"][4].items():
        assert torch.equal(res["1"][4][k], p0), k


def test_edge_offsets_that_do_not_match_the_edge_order_are_flagged():
    """the caller vouches for graph-sorted edges; an edge list in another order under the same offsets sets status bit 4
    (results are then unspecified); without the offsets any order is accepted"""
    batch = workloads.config2_batch(6)
    et = ("objects", "objects_to_objects", "objects")
    perm = torch.randperm(batch[et].edge_index.size(1), generator=torch.Generator().manual_seed(1))
    vouch = batch[et].ptr
    batch[et].edge_index = batch[et].edge_index[:, perm].contiguous()
    assert "ptr" not in batch[et], "a replaced edge_index must drop the offsets computed for the old one"
    batch[et].ptr = vouch  # a caller that (wrongly) vouches for the new list by hand
    with fuse_env("1"):
        _, net = build(SAGE_KW, HeterogeneousNetwork, omodels.HeterogeneousNetwork)
        net.eval()
        net(batch.to(DEV))
        assert net.native().read_state()[1] & 4
        # the same edges without the vouching offsets: accepted, and equal to the sorted batch's result
        ref_batch = workloads.config2_batch(6)
        _, net2 = build(SAGE_KW, HeterogeneousNetwork, omodels.HeterogeneousNetwork)
        net2.eval()
        want = net2(ref_batch.to(DEV))
        assert net2.native().read_state()[1] == 0
        del batch[et].ptr
        _, net3 = build(SAGE_KW, HeterogeneousNetwork, omodels.HeterogeneousNetwork)
        net3.eval()
        got = net3(batch.to(DEV))
        assert net3.native().read_state()[1] == 0
        torch.testing.assert_close(got, want, atol=1e-6, rtol=1e-6)


def _tiny_graph(rng, n_obj, n_room, feat=306):
    """a scene graph of a handful of nodes; any of the four edge lists may be empty, n_room may be 0"""
    from hydra_gnn_amd.data import HeteroData

    g = HeteroData()
    g["objects"].x = torch.from_numpy(rng.normal(0, 0.5, size=(n_obj, feat)).astype(np.float32))
    g["rooms"].x = torch.from_numpy(rng.normal(0, 0.5, size=(n_room, 6)).astype(np.float32))
    g["rooms"].y = torch.from_numpy(rng.integers(0, 26, size=n_room).astype(np.int64))

    def edges(n_src, n_dst, n):
        if n_src == 0 or n_dst == 0 or n == 0:
            return torch.zeros(2, 0, dtype=torch.int64)
        return torch.from_numpy(np.stack([rng.integers(0, n_src, size=n), rng.integers(0, n_dst, size=n)], 0).astype(np.int64))

    g["objects", "objects_to_objects", "objects"].edge_index = edges(n_obj, n_obj, int(rng.integers(0, 3 * n_obj + 1)))
    g["rooms", "rooms_to_rooms", "rooms"].edge_index = edges(n_room, n_room, int(rng.integers(0, 3)))
    g["objects", "objects_to_rooms", "rooms"].edge_index = edges(n_obj, n_room, int(rng.integers(0, n_obj + 1)))
    g["rooms", "rooms_to_objects", "objects"].edge_index = edges(n_room, n_obj, int(rng.integers(0, n_obj + 1)))
    return g


def test_plan_slices_with_many_tiny_graphs_and_empty_parts(monkeypatch):
    """1 300 graphs of 1-6 objects and 0-2 rooms (more graphs than threads of a plan part; graphs without rooms, without edges of
    a type; rows whose part boundary falls inside a graph): sliced and whole-list plan builds agree bit for bit, and with the oracle"""
    from hydra_gnn_amd.data import collate

    rng = np.random.Generator(np.random.PCG64(77))
    graphs = [_tiny_graph(rng, int(rng.integers(1, 7)), int(rng.integers(0, 3))) for _ in range(1300)]
    batch = collate(graphs)
    assert batch["rooms"].x.size(0) > 0 and int(batch["objects"].ptr[-1]) == batch["objects"].x.size(0)
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("HMP_PLAN_SLICED", mode)
        with fuse_env("1"):
            ora, net = build(SAGE_KW, HeterogeneousNetwork, omodels.HeterogeneousNetwork)
            res[mode] = run_fwd_bwd(net, batch, "rooms")
            assert net.native().read_state()[1] == 0
    monkeypatch.delenv("HMP_PLAN_SLICED")
    assert torch.equal(res["1"][0], res["0"][0])
    for k, g in res["0"][2].items():
        if g is not None:
            assert torch.equal(res["1"][2][k], g), k
    o64 = copy.deepcopy(ora).double()
    b64 = batch.to("cpu")
    for t in b64.node_types:
        b64[t].x = b64[t].x.double()
    pred_ref = o64(b64)
    y = batch["rooms"].y
    o64.loss(pred_ref, y, y != 25).backward()
    torch.testing.assert_close(res["1"][0].cpu().double(), pred_ref.detach(), atol=ATOL, rtol=RTOL)
    for name, p in o64.named_parameters():
        if p.grad is not None:
            torch.testing.assert_close(res["1"][2][name].cpu().double(), p.grad, atol=ATOL, rtol=RTOL, msg=lambda m: f"{name}: {m}")
