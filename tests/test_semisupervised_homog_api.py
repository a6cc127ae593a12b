"""CPU-side checks of the homogeneous two-headed fused step's interface: the ABI mirrors of hmp_linear_heads /
hmp_linear_head_targets, the head parameters' place in the flat buffer, the refusals, and workloads.stanford_semisupervised_batch."""
import ctypes as C

import pytest
import torch

from hydra_gnn_amd import _lib, workloads
from hydra_gnn_amd.models import HomogeneousNetwork, HomogeneousNeuralTreeNetwork

OUT = {"room": 15, "object": 35}
NEW = ("hmp_net_set_linear_heads", "hmp_net_step_heads_fwd_bwd", "hmp_net_step_heads_fused", "hmp_net_count_correct_heads")


def test_linear_head_mirrors_match_c_layout():
    lib = _lib.load()
    assert lib.hmp_abi_version() == _lib.ABI_VERSION == 4
    assert _lib._STRUCTS[8] is _lib.LinearHeads and _lib._STRUCTS[9] is _lib.LinearHeadTargets
    assert lib.hmp_sizeof(8) == C.sizeof(_lib.LinearHeads) == 48
    assert lib.hmp_sizeof(9) == C.sizeof(_lib.LinearHeadTargets) == 32
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES


@pytest.mark.parametrize("cls,block", [(HomogeneousNetwork, "GraphSAGE"), (HomogeneousNetwork, "GAT"),
                                       (HomogeneousNeuralTreeNetwork, "GAT_edge")])
def test_head_parameters_live_in_the_active_range(cls, block):
    kw = dict(input_dim=6, output_dim_dict=dict(OUT), conv_block=block, hidden_dim=30, num_layers=3, dropout=0.25,
              GAT_hidden_dims=[16, 16], GAT_heads=[6, 6], GAT_concats=[True, True])
    if cls is HomogeneousNeuralTreeNetwork:
        kw.update(disable_initialization=False)
    torch.manual_seed(1)
    net = cls(**kw)
    keys = list(net.state_dict())
    vals = {k: v.clone() for k, v in net.state_dict().items()}
    nn_ = net.native()
    heads = [net.post_mp_room.weight, net.post_mp_room.bias, net.post_mp_object.weight, net.post_mp_object.bias]
    assert [id(p) for p in nn_.head_params] == [id(p) for p in heads]
    for p in heads:
        off = nn_.param_offsets[id(p)]
        assert off % 4 == 0 and 0 <= off and off + p.numel() <= nn_.n_active
        assert all(p is not q for q in nn_.params)  # not among the parameters the autograd path returns gradients for
    for p, live in zip(nn_.params, nn_.param_active):  # dead weights stay past n_active
        if not live:
            assert nn_.param_offsets[id(p)] >= nn_.n_active
    assert nn_.tail[0] == (_lib.ACT_ELU if block != "GraphSAGE" else _lib.ACT_RELU) and nn_.tail[1] == pytest.approx(0.25)
    hd = nn_._linear_heads()
    assert hd.F == net.post_mp_room.in_features == nn_.layers[-1].out_dims["node"]
    assert list(hd.classes) == [15, 35]
    assert list(net.state_dict()) == keys
    assert all(torch.equal(net.state_dict()[k], v) for k, v in vals.items())


def test_single_output_layout_is_unchanged():
    net = HomogeneousNetwork(6, output_dim=15, conv_block="GraphSAGE", hidden_dim=16, num_layers=2)
    nn_ = net.native()
    assert nn_.heads is None and nn_.head_params == [] and nn_.tail == (_lib.ACT_NONE, 0.0)


def test_refusals():
    room = HomogeneousNetwork(6, output_dim=15, conv_block="GraphSAGE", hidden_dim=16, num_layers=2)
    with pytest.raises(_lib.HydraMPError):
        room.semisupervised_step(lr=1e-3)
    with pytest.raises(_lib.HydraMPError):
        room.count_correct(None)
    for block in ("GCN", "GIN"):
        op = HomogeneousNetwork(6, output_dim_dict=dict(OUT), conv_block=block, hidden_dim=16, num_layers=2)
        with pytest.raises(_lib.HydraMPError):
            op.semisupervised_step(lr=1e-3)
        with pytest.raises(_lib.HydraMPError):
            op.count_correct(None)
    two = HomogeneousNetwork(6, output_dim_dict=dict(OUT), conv_block="GraphSAGE", hidden_dim=16, num_layers=2)
    with pytest.raises(NotImplementedError):
        two.train_step(lr=1e-3)


def test_stanford_semisupervised_batch_split():
    b = workloads.stanford_semisupervised_batch(10, seed=3)
    c = workloads.stanford_semisupervised_batch(10, seed=3)
    tr, va, te = b.train_mask, b.val_mask, b.test_mask
    assert tr.dtype == torch.bool and tr.numel() == b.y.numel() == b.x.size(0)
    assert bool((tr.int() + va.int() + te.int() == 1).all())
    assert 0 < int(tr.sum()) and 0 < int(va.sum()) and 0 < int(te.sum())
    assert int(b.room_mask.sum()) == 10
    assert int(b.y[b.room_mask].max()) < 15 and int(b.y[~b.room_mask].max()) < 35
    assert torch.equal(tr, c.train_mask) and torch.equal(b.y, c.y)
