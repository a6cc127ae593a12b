"""K1 (csrc/aggregate.hip) -- the SAGE aggregation kernels -- at the shapes and edges the network parity tests do not reach.

Network level, against the float64 oracle with the same state_dict (logits, loss, every gradient; status word 0):
  * regime_batch (tests/_sage_regimes.py): every edge type has destinations of in-degree 0, 1, 7, 8, 9, 15, 16, 17, 24, 31, 32,
    33, 64, 65 and a hub of 320 and sources of the same out-degrees, so both directions cross every batch boundary of agg_row /
    agg_bwd_row (8-id batches, the GS <= 16 prefetch of ids 8..15, the 16-id batches of GS = 64, the UB = 8 / 4 tails); the two
    lists into one node type are empty / long on the same row (a pair with an empty partner), a room receives nothing;
  * hidden 32 .. 1000 under HMP_FUSE=0 and =1: every (GS, NV) instantiation, the fused projection at pK 48 / 208 and stacked
    widths not a multiple of 16; fpad(hidden) > 1024 is refused with HydraMPError;
  * the fused training step with the cross entropy in the last aggregation at GS 8 / 16 / 32 / 64, three steps against the
    oracle + torch.optim.Adam, and an out-of-range label flagged at each width;
  * training mode with dropout at GS 16 and 64, the 8-row-tile launch and the launch past 3584 rows, the homogeneous network
    (one edge type per destination) and the H-tree network (3 incoming types into room-room);
  * the LDS-window kernels (bf16 mode, 40 037 objects) on chunks over the 3072-id capacity in both directions and a hub of 2400
    in-neighbours, with and without the window kernels, against the bf16-contract oracle.
Unit level: hmp_segment_mean_fwd / _bwd on the regime edge lists at every (GS, NV) and both vector widths, against
pyg_ref.scatter_mean in float64, padding untouched.  The launch decisions are mirrored in tests/_sage_regimes.py and checked on the
host by tests/test_sage_dispatch.py.

Tolerance: 1e-5 (atol + rtol) against float64, as in test_gpu_models.py.
"""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _sage_regimes as R  # noqa: E402
from hydra_gnn_amd import _lib, workloads  # noqa: E402
from hydra_gnn_amd.data import HTREE_EDGE_TYPES, Data  # noqa: E402
from hydra_gnn_amd.models import HeterogeneousNetwork, HeterogeneousNeuralTreeNetwork, HomogeneousNetwork  # noqa: E402
from oracle import models as omodels  # noqa: E402
from oracle import pyg_ref  # noqa: E402
from test_gpu_config5 import bf16_contract, check_against_bf16_contract, make_replay  # noqa: E402
from test_gpu_fusion import build, fuse_env  # noqa: E402
from test_gpu_htree import HT_DIMS, compare, to64  # noqa: E402
from test_gpu_models import assert_grads_close, oracle_run  # noqa: E402
from test_gpu_ops import build_plan  # noqa: E402

ATOL, RTOL = 1e-5, 1e-5
DEV = "cuda:0"
NAN = float("nan")


def sage_kw(hidden, out_dim=26, dropout=0.0, layers=3):
    return dict(input_dim_dict=dict(R.MP3D_IN_DIMS), output_dim=out_dim, conv_block="GraphSAGE", hidden_dim=hidden,
                num_layers=layers, dropout=dropout)


_BATCHES = {}


def regime(copies=1):
    if copies not in _BATCHES:
        b = R.regime_batch(copies)
        R.check_sage_regimes(b)
        _BATCHES[copies] = b
    return _BATCHES[copies]


def eval_parity(ora, net, batch):
    """eval forward + loss + backward of the engine against oracle_run (float64), status word 0"""
    o64, pred_ref, loss_ref = oracle_run(ora, batch)
    net.eval()
    pred = net(batch.to(DEV))
    torch.testing.assert_close(pred.cpu().double(), pred_ref, atol=ATOL, rtol=RTOL)
    y = batch["rooms"].y.to(DEV)
    loss = net.loss(pred, y, y != 25)
    torch.testing.assert_close(loss.cpu().double(), loss_ref, atol=ATOL, rtol=RTOL)
    loss.backward()
    assert_grads_close(net, o64)
    assert net.native().read_state()[1] == 0


# =================================================================================================
# every row-group class on the degree regimes
# =================================================================================================
@pytest.mark.parametrize("fuse", ["0", "1"])
@pytest.mark.parametrize("hidden", R.HIDDEN_CASES)
def test_hetero_sage_parity_on_degree_regimes(hidden, fuse):
    """hidden <= 256 with HMP_FUSE=1: the fused projection / input-gradient kernels at GS 16 / 32 / 64 (pK 48 and 208 are not
    multiples of 64, the stacked widths of the last layer -- 28 and 56 -- not multiples of 16); hidden > 256: the stand-alone
    kernels at NV = 2, 2, 3, 4 in both sequences."""
    batch = regime()
    nn, ne = R.batch_sizes(batch)
    shapes = {(d["kernel"], d["gs"], d["nv"]) for d in R.hetero_sage_launches(hidden, 26, 3, fuse == "1", nn, ne)}
    print(f"hidden {hidden}, HMP_FUSE={fuse}: {sorted(shapes)}")
    with fuse_env(fuse):
        ora, net = build(sage_kw(hidden), HeterogeneousNetwork, omodels.HeterogeneousNetwork, seed=hidden)
        eval_parity(ora, net, batch)


@pytest.mark.parametrize("fuse", ["0", "1"])
def test_unsupported_width_is_refused(fuse):
    """fpad(hidden) = 1028 needs 5 float4 chunks per lane of a 64-lane row group: no instantiation; the launch must refuse it
    with HydraMPError (no crash, no numbers)."""
    assert R.pick_shape(R.fpad(R.UNSUPPORTED_HIDDEN)) not in R.AGG_SHAPES
    with fuse_env(fuse):
        _, net = build(sage_kw(R.UNSUPPORTED_HIDDEN), HeterogeneousNetwork, omodels.HeterogeneousNetwork)
        net.eval()
        with pytest.raises(_lib.HydraMPError):
            net(regime().to(DEV))
            torch.cuda.synchronize()


# =================================================================================================
# the masked cross entropy in the last aggregation at every row-group width
# =================================================================================================
def ce_labels(batch, out_dim, seed):
    """labels over every class (so the row maximum and the hit sit in any lane of the row group), a seventh ignored (25)"""
    rng = np.random.default_rng(seed)
    n = int(batch["rooms"].x.size(0))
    y = rng.integers(0, out_dim, size=n)
    y[rng.random(n) < 1 / 7] = 25
    return torch.from_numpy(y.astype(np.int64))


@pytest.mark.parametrize("out_dim", R.CE_OUT_DIMS)
def test_fused_cross_entropy_at_every_row_group_width(out_dim):
    """fused training step (plan + forward + CE in the epilogue of the last aggregation + backward + Adam), 3 steps, against the
    float64 oracle + torch.optim.Adam (the acceptance rule of test_fused_train_step_matches_oracle_adam); then an out-of-range
    label sets status bit 2."""
    batch = regime()
    nn, ne = R.batch_sizes(batch)
    ce = [d for d in R.hetero_sage_launches(R.CE_HIDDEN, out_dim, 3, True, nn, ne, ce=True) if d["ce"]]
    assert len(ce) == 1
    print(f"out_dim {out_dim}: cross entropy at GS {ce[0]['gs']}")
    y = ce_labels(batch, out_dim, out_dim)
    steps, lr, wd = 3, 0.002, 0.001
    with fuse_env("1"):
        ora, net = build(sage_kw(R.CE_HIDDEN, out_dim), HeterogeneousNetwork, omodels.HeterogeneousNetwork, seed=out_dim)
        o64 = copy.deepcopy(ora).double()
        opt = torch.optim.Adam(o64.parameters(), lr=lr, weight_decay=wd)
        b64 = batch.to("cpu")
        for t in b64.node_types:
            b64[t].x = b64[t].x.double()
        losses_ref = []
        tiny = {n: torch.zeros_like(p, dtype=torch.bool) for n, p in o64.named_parameters()}
        for _ in range(steps):
            opt.zero_grad()
            loss = o64.loss(o64(b64), y, y != 25)
            loss.backward()
            for n, p in o64.named_parameters():
                if p.grad is not None:
                    tiny[n] |= p.grad.abs() < 1e-5
            opt.step()
            losses_ref.append(float(loss.detach()))
        step = net.train_step(lr=lr, weight_decay=wd, ignored_label=25, use_graph=False)
        gb = batch.to(DEV)
        yg = y.to(DEV)
        losses = []
        for _ in range(steps):
            step(gb, yg)
            losses.append(step.loss())
        np.testing.assert_allclose(losses, losses_ref, rtol=2e-5, atol=2e-5)
        ref = dict(o64.named_parameters())
        n_tiny = n_all = 0
        for name, p in net.named_parameters():
            ok = ~tiny[name]
            n_tiny += int(tiny[name].sum()); n_all += tiny[name].numel()
            diff = (p.detach().cpu().double() - ref[name].detach()).abs()
            if bool(ok.any()):
                assert float(diff[ok].max()) <= 1e-3, name
                assert float((diff[ok] > 5e-5).double().mean()) < 0.01, name
            assert float(diff.max()) <= steps * lr * 2.1, name
        assert n_tiny < 0.2 * n_all
        st, status = net.native().read_state()
        assert st == steps and status == 0
        bad = y.clone()
        bad[int(torch.nonzero(y != 25)[0])] = out_dim
        step(gb, bad.to(DEV))
        assert net.native().read_state()[1] & 2


# =================================================================================================
# training mode, launch shape, single-type and many-type pairing
# =================================================================================================
@pytest.mark.parametrize("hidden", R.DROPOUT_HIDDEN)
def test_dropout_training_parity_on_degree_regimes(hidden):
    """training mode, dropout 0.25, the oracle replaying the engine's keep-masks (as test_dropout_training_parity_with_replayed_masks)"""
    batch = regime()
    ora, net = build(sage_kw(hidden, dropout=0.25), HeterogeneousNetwork, omodels.HeterogeneousNetwork, seed=hidden + 1)
    net.train()
    pred = net(batch.to(DEV))
    ora.dropout_fn = make_replay(net)
    o64, pred_ref, loss_ref = oracle_run(ora, batch, train=True)
    torch.testing.assert_close(pred.cpu().double(), pred_ref, atol=ATOL, rtol=RTOL)
    y = batch["rooms"].y.to(DEV)
    loss = net.loss(pred, y, y != 25)
    torch.testing.assert_close(loss.cpu().double(), loss_ref, atol=ATOL, rtol=RTOL)
    loss.backward()
    assert_grads_close(net, o64)
    assert net.native().read_state()[1] == 0


@pytest.mark.parametrize("copies", R.LAUNCH_COPIES)
def test_launch_shape_tiles_of_eight_and_none(copies):
    """the regime scene alone is a small launch whose room entries (> 8 edges per room both ways) run 8-row tiles; ten copies
    put every launch past 3584 rows (and 224 tiles of 16), where the tiles are off"""
    batch = regime(copies)
    nn, ne = R.batch_sizes(batch)
    tile8 = {d["kernel"] for d in R.hetero_sage_launches(R.LAUNCH_HIDDEN, 26, 3, True, nn, ne) if d["tile8"]}
    if copies == 1:
        assert {"agg_fwd_kernel", "agg_proj_fwd_kernel", "agg_bwd_dx_kernel"} <= tile8, tile8
    else:
        assert not tile8, tile8
    with fuse_env("1"):
        ora, net = build(sage_kw(R.LAUNCH_HIDDEN), HeterogeneousNetwork, omodels.HeterogeneousNetwork, seed=copies)
        eval_parity(ora, net, batch)


@pytest.mark.parametrize("hidden", [64, 300])
def test_homogeneous_sage_parity_on_degree_regimes(hidden):
    """one edge type per destination: every pair of agg_row has no partner (has2 = false)"""
    torch.manual_seed(hidden)
    kw = dict(input_dim=6, output_dim=15, conv_block="GraphSAGE", hidden_dim=hidden, num_layers=3, dropout=0.0)
    ora = omodels.HomogeneousNetwork(**kw)
    net = HomogeneousNetwork(**kw)
    net.load_state_dict(ora.state_dict(), strict=True)
    net = net.to(DEV).eval()
    rng = np.random.default_rng(hidden)
    x, ei, room_mask = R.homogeneous_regime_graph(rng)
    n = x.size(0)
    din, dout = torch.bincount(ei[1], minlength=n), torch.bincount(ei[0], minlength=n)
    assert set(R.DEG_CLASSES) <= set(din.tolist()) and set(R.DEG_CLASSES) <= set(dout.tolist())
    y = torch.from_numpy(rng.integers(0, 15, size=n).astype(np.int64))
    o64 = copy.deepcopy(ora).double().eval()
    ref = o64(Data(x=x.double(), edge_index=ei, room_mask=room_mask))
    out = net(Data(x=x, edge_index=ei, room_mask=room_mask, y=y).to(DEV))
    torch.testing.assert_close(out.detach().cpu().double(), ref.detach(), atol=ATOL, rtol=RTOL)
    yr = y[room_mask]
    loss_ref = o64.loss(ref, yr)
    loss_ref.backward()
    loss = net.loss(out, yr.to(DEV))
    torch.testing.assert_close(loss.detach().cpu().double(), loss_ref.detach(), atol=ATOL, rtol=RTOL)
    loss.backward()
    og = dict(o64.named_parameters())
    for name, q in net.named_parameters():
        assert q.grad is not None, name
        torch.testing.assert_close(q.grad.cpu().double(), og[name].grad, atol=ATOL, rtol=RTOL, msg=lambda m: f"{name}: {m}")
    assert net.native().read_state()[1] == 0


@pytest.mark.parametrize("fuse", ["0", "1"])
def test_htree_sage_parity_with_odd_incoming_type_counts(fuse):
    """room-room receives 3 edge types (a pair and a single), object 1: the pairs of agg_row with and without a partner"""
    batch = workloads.htree_batch(7, seed=41)
    n_in = {}  # node type -> incoming edge types that carry edges in this batch
    for et in HTREE_EDGE_TYPES:
        if batch[et].edge_index.size(1) > 0:
            n_in[et[2]] = n_in.get(et[2], 0) + 1
    assert n_in.get("room-room") == 3 and n_in.get("object") == 1, n_in
    torch.manual_seed(3)
    kw = dict(input_dim_dict=HT_DIMS, output_dim=26, conv_block="GraphSAGE", hidden_dim=48, num_layers=3,
              disable_initialization=True, dropout=0.0)
    with fuse_env(fuse):
        ora = omodels.HeterogeneousNeuralTreeNetwork(**kw)
        net = HeterogeneousNeuralTreeNetwork(**kw)
        net.load_state_dict(ora.state_dict(), strict=True)
        net = net.to(DEV).eval()
        o64 = copy.deepcopy(ora).double().eval()
        pred_ref = o64(to64(batch))
        pred = net(batch.to(DEV))
        compare(net, o64, pred, pred_ref, batch["room_virtual"].y)
        assert net.native().read_state()[1] == 0


# =================================================================================================
# unit: hmp_segment_mean_fwd / _bwd
# =================================================================================================
@pytest.mark.parametrize("F,pad_in,pad_out", R.SEGMENT_CASES)
def test_segment_mean_on_regime_edge_lists(F, pad_in, pad_out):
    """every edge list of the regime batch; the padding columns of the outputs keep their NaN"""
    lib = _lib.require_device()
    batch = regime()
    print(f"F {F}, ld +{pad_in} / +{pad_out}: {R.segment_shape(F, pad_in, pad_out)}")
    rng = np.random.default_rng(F + pad_in)
    for et in R.MP3D_EDGE_TYPES:
        ei = batch[et].edge_index
        n_src, n_dst = int(batch[et[0]].x.size(0)), int(batch[et[2]].x.size(0))
        plan = build_plan(ei.to(DEV), n_src, n_dst)
        assert plan["status"] == 0
        x = torch.from_numpy(rng.normal(size=(n_src, F)))
        g = torch.from_numpy(rng.normal(size=(n_dst, F)))
        ldx, ldo = F + pad_in, F + pad_out
        xd = torch.full((n_src, ldx), NAN); xd[:, :F] = x.float(); xd = xd.to(DEV)
        gd = torch.full((n_dst, ldx), NAN); gd[:, :F] = g.float(); gd = gd.to(DEV)
        out = torch.full((n_dst, ldo), NAN, device=DEV)
        gx = torch.full((n_src, ldo), NAN, device=DEV)
        _lib.check(lib.hmp_segment_mean_fwd(xd.data_ptr(), ldx, F, plan["plan"], out.data_ptr(), ldo, _lib.stream_ptr()))
        _lib.check(lib.hmp_segment_mean_bwd(gd.data_ptr(), ldx, F, plan["plan"], gx.data_ptr(), ldo, _lib.stream_ptr()))
        torch.cuda.synchronize()
        x64 = x.float().double().requires_grad_(True)
        ref = pyg_ref.scatter_mean(x64[ei[0]], ei[1], n_dst)
        (ref * g.float().double()).sum().backward()
        out, gx = out.cpu(), gx.cpu()
        torch.testing.assert_close(out[:, :F].double(), ref.detach(), atol=ATOL, rtol=RTOL, msg=lambda m: f"{et[1]} fwd: {m}")
        torch.testing.assert_close(gx[:, :F].double(), x64.grad, atol=ATOL, rtol=RTOL, msg=lambda m: f"{et[1]} bwd: {m}")
        assert torch.isnan(out[:, F:]).all() and torch.isnan(gx[:, F:]).all(), f"{et[1]}: a padding column was written"


# =================================================================================================
# LDS-window kernels at their edges
# =================================================================================================
@pytest.fixture(scope="module")
def win_graph():
    g = R.window_graph()
    R.check_window_graph(g)
    return g


def test_lds_window_kernels_over_capacity_and_hub_against_the_bf16_contract(win_graph, monkeypatch):
    """bf16 mode, hidden 256, dropout 0.25, training mode, 40 037 objects (a partial last chunk): window chunks of 64 rows over
    the 3072 staged ids in both directions (their rows of > 64 ids read extents and ids from global memory: the !fits path);
    in chunks that fit, rows of > 64 ids walked 64 staged ids at a time -- three rows of ~107 and a hub of 2400 in-neighbours
    whose chunk is thinned so that it fits, half of them inside the LDS ring (chunk +- 64 rows) and half read through buffer
    loads -- and in the backward pass a fan-out source of 1500; objects whose only neighbour is their room.  (check_window_graph
    asserts each of these on the graph.)  With the window kernels and without (HMP_AGG_WIN=0), each run against oracle/bf16_emul.py's contract by the rule
    of test_config5_bf16_mode_matches_the_bf16_contract_oracle.  (With a hub the two runs associate a long fp32 sum differently:
    bit identity is not expected here and not asserted.)"""
    monkeypatch.setenv("HMP_BF16_ALL", "1")
    monkeypatch.setenv("HMP_FUSE", "0")
    kw = dict(input_dim_dict={"objects": 256, "rooms": 256}, output_dim=26, conv_block="GraphSAGE", hidden_dim=256, num_layers=3,
              dropout=0.25)
    ora, net = build(kw, HeterogeneousNetwork, omodels.HeterogeneousNetwork, seed=1)
    net.native().set_compute("bf16")
    g = win_graph.to(DEV)
    y = g["rooms"].y

    def fwd_bwd():
        net._rng_step = 0
        for p in net.parameters():
            p.grad = None
        net.train()
        pred = net(g)
        loss = net.loss(pred, y, y != 25)
        loss.backward()
        assert net.native().read_state()[1] == 0
        return (pred.detach().cpu().clone(), float(loss),
                {k: (p.grad.detach().cpu().clone() if p.grad is not None else None) for k, p in net.named_parameters()})

    runs = {"window": fwd_bwd()}
    monkeypatch.setenv("HMP_AGG_WIN", "0")
    runs["plain"] = fwd_bwd()
    monkeypatch.delenv("HMP_AGG_WIN")
    replay = make_replay(net)  # both runs drew the masks of rng step 1
    nat = net.native()
    af = {(l, tuple(nat.layers[l].convs[c].edge_type)) for (l, c), on in nat._agg_first.items() if on}
    assert af == {(l, ("objects", "objects_to_rooms", "rooms")) for l in range(3)}, af
    contract = bf16_contract(ora, win_graph, replay, af)
    for what, (pred, loss, grads) in runs.items():
        report = check_against_bf16_contract(contract, pred, loss, grads)
        worst = max(report[1:], key=lambda r: r[1])
        print(f"{what}: logits {report[0][1]:.2e} (spread {report[0][2]:.2e}), worst gradient {worst[0]} {worst[1]:.2e}")
