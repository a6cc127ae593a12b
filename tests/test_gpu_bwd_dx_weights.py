"""The fused input gradient (csrc/aggregate.hip agg_bwd_dx_tile) on the transposed weight image the pack writes (PackSeg::dst_t).

HeterogeneousNetwork(GraphSAGE), 3 layers, output 26, HMP_FUSE=1, against the float64 oracle with the same state_dict (logits, loss,
every gradient; status word 0), at the widths where the 16-wide column tiles and the 16-deep k blocks of that GEMM have edges:
  * hidden 16: one column tile (three of the four waves have none, and prefetch nothing); stacked width K = 48;
  * hidden 20: xN = 20 and K = 60 are not multiples of 16 -- a partial column tile with clamped rows of the image, a last k block
    that meets the zero rows of the LDS image and the zero padding columns of WpT; the forward projection is not fused at this
    width, the input gradient is;
  * hidden 36: three column tiles, the last partial; K = 108;
each on the degree-regime batch (tests/_sage_regimes.py: 8-row tiles, the last layer's stacked widths 28 / 56) and on a batch of
two MP3D-like graphs whose room entry has fewer than 16 rows (masked tile rows);
  * hidden 300: the stand-alone kernels -- nothing may ask for the image where it is not read;
  * training mode, dropout 0.25, hidden 20, the oracle replaying the engine's keep-masks: the sign-of-zero keep bit and the
    activation derivative in the epilogue.

Tolerance: 1e-5 (atol + rtol) against float64, as in test_gpu_sage_kernels.py.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _sage_regimes as R  # noqa: E402
from hydra_gnn_amd import workloads  # noqa: E402
from hydra_gnn_amd.models import HeterogeneousNetwork  # noqa: E402
from oracle import models as omodels  # noqa: E402
from test_gpu_config5 import make_replay  # noqa: E402
from test_gpu_fusion import build, fuse_env  # noqa: E402
from test_gpu_models import assert_grads_close, oracle_run  # noqa: E402

ATOL, RTOL = 1e-5, 1e-5
DEV = "cuda:0"

_BATCHES = {}


def batch_of(name):
    if name not in _BATCHES:
        if name == "regime":
            b = R.regime_batch()
            R.check_sage_regimes(b)
        else:
            b = workloads.mp3d_like_batch(2, seed=23)
            assert 0 < int(b["rooms"].x.size(0)) < 16
        _BATCHES[name] = b
    return _BATCHES[name]


def sage_kw(hidden, dropout=0.0):
    return dict(input_dim_dict=dict(R.MP3D_IN_DIMS), output_dim=26, conv_block="GraphSAGE", hidden_dim=hidden, num_layers=3,
                dropout=dropout)


def eval_parity(ora, net, batch):
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


@pytest.mark.parametrize("which", ["regime", "two_graphs"])
@pytest.mark.parametrize("hidden", [16, 20, 36])
def test_input_gradient_at_column_tile_and_k_block_edges(hidden, which):
    batch = batch_of(which)
    if which == "regime":
        nn, ne = R.batch_sizes(batch)
        kernels = {d["kernel"] for d in R.hetero_sage_launches(hidden, 26, 3, True, nn, ne)}
        assert "agg_bwd_dx_kernel" in kernels, kernels
    with fuse_env("1"):
        ora, net = build(sage_kw(hidden), HeterogeneousNetwork, omodels.HeterogeneousNetwork, seed=hidden)
        eval_parity(ora, net, batch)


def test_stand_alone_kernels_do_not_need_the_image():
    batch = batch_of("regime")
    nn, ne = R.batch_sizes(batch)
    bwd = {d["layer"]: d["kernel"] for d in R.hetero_sage_launches(300, 26, 3, True, nn, ne) if d["kernel"].startswith("agg_bwd")}
    # layer 1 gathers 300-wide segments: stand-alone kernels; the last layer's (28 wide) is fused, 19 column tiles over xN = 300
    assert bwd == {0: "agg_bwd_kernel", 1: "agg_bwd_kernel", 2: "agg_bwd_dx_kernel"}, bwd
    with fuse_env("1"):
        ora, net = build(sage_kw(300), HeterogeneousNetwork, omodels.HeterogeneousNetwork, seed=300)
        eval_parity(ora, net, batch)


def test_dropout_training_parity_at_hidden_20():
    """as test_gpu_sage_kernels.test_dropout_training_parity_on_degree_regimes"""
    batch = batch_of("regime")
    with fuse_env("1"):
        ora, net = build(sage_kw(20, dropout=0.25), HeterogeneousNetwork, omodels.HeterogeneousNetwork, seed=21)
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
