"""CPU checks of the room-task validation count's interface: the new C entries are exported and bound, two-headed models refuse
count_correct_rooms, and evaluate.accuracy_matrix assembles the reference's (C - 1) x C matrix (base_training_job.py:275-308)
from a confusion matrix."""
import numpy as np
import pytest
import torch

from hydra_gnn_amd import _lib, evaluate, ops
from hydra_gnn_amd.data import HTREE_NODE_TYPES
from hydra_gnn_amd.models import (HeterogeneousNetwork, HeterogeneousNeuralTreeNetwork, HomogeneousNetwork,
                                  HomogeneousNeuralTreeNetwork)

HT_DIMS = {"object": 306, "room": 6, "object-room": 6, "room-room": 6, "object_virtual": 306, "room_virtual": 6}


def test_new_entries_are_exported_and_bound():
    lib = _lib.load()
    for name in ("hmp_count_correct_rows", "hmp_net_count_correct_rooms"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.hmp_abi_version() == 4
    assert callable(ops.count_correct_rows) and callable(evaluate.accuracy)
    for cls in (HeterogeneousNetwork, HeterogeneousNeuralTreeNetwork, HomogeneousNetwork, HomogeneousNeuralTreeNetwork):
        assert callable(getattr(cls, "count_correct_rooms", None)), cls.__name__


def test_operator_has_no_cpu_path():
    with pytest.raises(_lib.HydraMPError):
        ops.count_correct_rows(torch.zeros(3, 4), torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int64))


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a box WITHOUT a GPU")
def test_entry_points_refuse_without_a_device():
    lib = _lib.load()
    assert lib.hmp_count_correct_rows(None, 4, 0, 4, None, None, 25, None, None, None) == 0  # nothing to count: no launch
    assert lib.hmp_count_correct_rows(None, 4, 3, 4, None, None, 25, None, None, None) != 0
    assert lib.hmp_net_count_correct_rooms(None, None, None, None, 25, None, None, None) != 0


def two_headed_models():
    yield HeterogeneousNetwork({"objects": 306, "rooms": 6}, output_dim_dict={"rooms": 26, "objects": 10}, conv_block="GraphSAGE",
                               hidden_dim=8, num_layers=2)
    yield HeterogeneousNeuralTreeNetwork(HT_DIMS, output_dim_dict={**{t: 10 for t in HTREE_NODE_TYPES}, "room": 26}, conv_block="GraphSAGE",
                                         hidden_dim=8, num_layers=2, disable_initialization=True)
    yield HomogeneousNetwork(6, output_dim_dict={"rooms": 15, "objects": 20}, conv_block="GraphSAGE", hidden_dim=8, num_layers=2)
    yield HomogeneousNeuralTreeNetwork(6, output_dim_dict={"room": 15, "object": 20}, conv_block="GraphSAGE", hidden_dim=8,
                                       num_layers=2, disable_initialization=True)


@pytest.mark.parametrize("i", range(4))
def test_two_headed_models_refuse_count_correct_rooms(i):
    model = list(two_headed_models())[i]
    with pytest.raises(_lib.HydraMPError, match="count_correct"):
        model.count_correct_rooms(None)


def reference_matrix(pred, label, ignored, C):
    """base_training_job.py:275-278 and 286-308 on CPU tensors, one batch"""
    num_valid_rooms = C - 1
    accuracy_matrix = np.zeros((num_valid_rooms, num_valid_rooms + 1), dtype=int)
    mask = label != ignored
    pred, label = pred[mask], label[mask]
    for l in range(num_valid_rooms):
        if l == ignored:
            continue
        for ll in range(num_valid_rooms + 1):
            accuracy_matrix[l, ll] = (pred[label == l] == ll).sum().item()
    return accuracy_matrix


@pytest.mark.parametrize("C,ignored", [(26, 25), (26, 3), (26, -100), (15, 25), (15, 0), (2, 0), (2, 1)])
def test_accuracy_matrix_equals_the_reference_double_loop(C, ignored):
    g = torch.Generator().manual_seed(C * 100 + ignored)
    n = 3000
    pred = torch.randint(0, C, (n,), generator=g)
    label = torch.randint(-1, C + 1, (n,), generator=g)
    label[::7] = ignored
    # the device's confusion matrix: counted rows (label != ignored) with label in [0, C), [label, pred] += 1
    keep = (label != ignored) & (label >= 0) & (label < C)
    conf = torch.bincount(label[keep] * C + pred[keep], minlength=C * C)
    got = evaluate.accuracy_matrix(conf, ignored)
    want = reference_matrix(pred, label, ignored, C)
    assert got.shape == (C - 1, C) and got.dtype == want.dtype
    assert np.array_equal(got, want)
    assert np.array_equal(evaluate.accuracy_matrix(conf.view(C, C).numpy(), ignored), want)
    if 0 <= ignored < C - 1:
        assert not got[ignored].any()
