"""CPU-side checks of the two-headed fused step's interface: the ABI mirror of hmp_head_targets, the refusal on a room-task
model, and the seeded train / val / test split of ``workloads.semisupervised_batch``."""
import ctypes as C

import pytest
import torch

from hydra_gnn_amd import _lib, workloads
from hydra_gnn_amd.models import HeterogeneousNetwork


def test_head_targets_mirror_matches_c_layout():
    lib = _lib.load()
    assert _lib._STRUCTS[7] is _lib.HeadTargets
    assert lib.hmp_sizeof(7) == C.sizeof(_lib.HeadTargets) == 32
    assert lib.hmp_abi_version() == _lib.ABI_VERSION == 4
    for name in ("hmp_net_step2_fwd_bwd", "hmp_net_step2_fused", "hmp_net_count_correct2"):
        assert hasattr(lib, name)


def test_semisupervised_step_refuses_a_room_task_model():
    net = HeterogeneousNetwork({"objects": 306, "rooms": 6}, output_dim=26, conv_block="GraphSAGE", hidden_dim=8, num_layers=2)
    with pytest.raises(_lib.HydraMPError):
        net.semisupervised_step(lr=1e-3)
    with pytest.raises(_lib.HydraMPError):
        net.count_correct(None, None)


def test_two_head_model_describes_its_tail():
    kw = dict(input_dim_dict={"objects": 306, "rooms": 6}, output_dim_dict={"rooms": 26, "objects": 28}, num_layers=2)
    sage = HeterogeneousNetwork(conv_block="GraphSAGE", hidden_dim=8, dropout=0.3, **kw)
    assert sage.native().tail == (_lib.ACT_RELU, pytest.approx(0.3))
    sp = sage.native()._spec()
    assert sp.tail_act == _lib.ACT_RELU and abs(sp.tail_dropout - 0.3) < 1e-7
    gat = HeterogeneousNetwork(conv_block="GAT", GAT_hidden_dims=[8], GAT_heads=[1, 1], GAT_concats=[True, False], dropout=0.1, **kw)
    assert gat.native().tail[0] == _lib.ACT_ELU
    room = HeterogeneousNetwork({"objects": 306, "rooms": 6}, output_dim=26, conv_block="GraphSAGE", hidden_dim=8, num_layers=2)
    assert room.native()._spec().tail_act == _lib.ACT_NONE


def test_semisupervised_batch_split():
    b = workloads.semisupervised_batch(6, seed=3)
    c = workloads.semisupervised_batch(6, seed=3)
    for t, n_cls in (("rooms", 26), ("objects", 28)):
        tr, va, te = b[t].train_mask, b[t].val_mask, b[t].test_mask
        assert tr.dtype == torch.bool and tr.numel() == b[t].y.numel()
        assert bool((tr.int() + va.int() + te.int() == 1).all())  # disjoint and covering
        assert 0 < int(tr.sum()) and 0 < int(va.sum()) and 0 < int(te.sum())
        assert int(b[t].y.min()) >= 0 and int(b[t].y.max()) < n_cls
        assert torch.equal(tr, c[t].train_mask) and torch.equal(b[t].y, c[t].y)
