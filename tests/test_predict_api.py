"""CPU checks of the label-prediction interface: the six new C entries are exported and bound with their argument types, no public
struct changed size (the entries are ABI-4-compatible additions), the models refuse to predict without a device (there is no CPU
fallback), and evaluate.predict rejects a malformed `batches` argument before it touches the device."""
import ctypes as C

import pytest
import torch

from hydra_gnn_amd import _lib, engine, evaluate, jobs, ops
from hydra_gnn_amd.data import HTREE_NODE_TYPES
from hydra_gnn_amd.models import (HeterogeneousNetwork, HeterogeneousNeuralTreeNetwork, HomogeneousNetwork,
                                  HomogeneousNeuralTreeNetwork)

HT_DIMS = {"object": 306, "room": 6, "object-room": 6, "room-room": 6, "object_virtual": 306, "room_virtual": 6}
VP, I32 = C.c_void_p, C.c_int32

NEW_ENTRIES = {
    "hmp_predict_rows": [VP, I32, I32, I32, VP, VP, VP],
    "hmp_head_tails_predict": [C.POINTER(_lib.TailDesc), I32, I32, I32, C.POINTER(VP), VP],
    "hmp_linear_heads_predict": [C.POINTER(_lib.LinearHeadsDesc), C.POINTER(VP), C.POINTER(I32), VP],
    "hmp_net_predict_rooms": [VP, C.POINTER(_lib.Batch), VP, VP, VP, VP],
    "hmp_net_predict2": [VP, C.POINTER(_lib.Batch), VP, C.POINTER(VP), VP],
    "hmp_net_predict_heads": [VP, C.POINTER(_lib.Batch), VP, C.POINTER(VP), C.POINTER(VP), VP],
}

# hmp_sizeof(i) of the public structs before the label entries were added, in _lib._STRUCTS order
STRUCT_BYTES = {"Plan": 64, "GatArgs": 40, "ConvSpec": 112, "LayerSpec": 1872, "NetSpec": 15184, "Batch": 736, "TrainArgs": 56,
                "HeadTargets": 32, "LinearHeads": 48, "LinearHeadTargets": 32, "GemmDesc": 128, "EpochCtl": 40, "EpochRow": 40,
                "EpochSeg": 24, "TailDesc": 128, "LinearHeadsDesc": 168, "PlanJob": 120, "FrontSeg": 40,
                "FrontProb": 280, "PackSeg": 128}


def test_new_entries_are_exported_and_bound():
    lib = _lib.load()
    for name, argtypes in NEW_ENTRIES.items():
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert name in _lib.SIGNATURES, name
        assert _lib.SIGNATURES[name][0] is C.c_int and list(_lib.SIGNATURES[name][1]) == argtypes, name
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name


def test_no_public_struct_changed_size():
    lib = _lib.load()
    assert lib.hmp_abi_version() == 4
    assert [st.__name__ for st in _lib._STRUCTS] == list(STRUCT_BYTES)
    for i, st in enumerate(_lib._STRUCTS):
        assert lib.hmp_sizeof(i) == STRUCT_BYTES[st.__name__] == C.sizeof(st), st.__name__


def test_python_surface_exists():
    assert callable(engine.NativeNet.predict_labels) and callable(engine.NativeNet.predict_pair)
    assert callable(evaluate.predict) and callable(ops.predict_rows)
    assert callable(jobs.BaseTrainingJob.predict) and callable(jobs.SemiSupervisedTrainingJob.predict)
    for cls in (HeterogeneousNetwork, HeterogeneousNeuralTreeNetwork, HomogeneousNetwork, HomogeneousNeuralTreeNetwork):
        assert callable(getattr(cls, "predict_labels", None)) and callable(getattr(cls, "predict", None)), cls.__name__


def models():
    two = dict(conv_block="GraphSAGE", hidden_dim=8, num_layers=2)
    yield HeterogeneousNetwork({"objects": 306, "rooms": 6}, output_dim=26, **two)
    yield HeterogeneousNetwork({"objects": 306, "rooms": 6}, output_dim_dict={"rooms": 26, "objects": 10}, **two)
    yield HeterogeneousNeuralTreeNetwork(HT_DIMS, output_dim_dict={**{t: 10 for t in HTREE_NODE_TYPES}, "room": 26},
                                         disable_initialization=True, **two)
    yield HomogeneousNetwork(6, output_dim=26, **two)
    yield HomogeneousNetwork(6, output_dim_dict={"rooms": 15, "objects": 20}, **two)
    yield HomogeneousNetwork(6, output_dim_dict={"rooms": 15, "objects": 20}, conv_block="GCN", hidden_dim=8, num_layers=2)
    yield HomogeneousNeuralTreeNetwork(6, output_dim_dict={"room": 15, "object": 20}, disable_initialization=True, **two)


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a box WITHOUT a GPU")
@pytest.mark.parametrize("i", range(7))
def test_predict_labels_refuses_without_a_device(i):
    model = list(models())[i]
    with pytest.raises(_lib.HydraMPError, match="no CPU fallback"):
        model.predict_labels(None)


def test_operator_has_no_cpu_path():
    with pytest.raises(_lib.HydraMPError):
        ops.predict_rows(torch.zeros(3, 4))


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a box WITHOUT a GPU")
def test_entry_points_refuse_without_a_device():
    lib = _lib.load()
    assert lib.hmp_predict_rows(None, 4, 0, 4, None, None, None) == 0  # no rows: no launch
    assert lib.hmp_predict_rows(None, 4, 3, 4, None, None, None) != 0
    assert lib.hmp_net_predict_rooms(None, None, None, None, None, None) != 0
    assert lib.hmp_net_predict2(None, None, None, None, None) != 0
    assert lib.hmp_net_predict_heads(None, None, None, None, None, None) != 0
    assert lib.hmp_head_tails_predict(None, 1, 0, 0, None, None) != 0
    assert lib.hmp_linear_heads_predict(None, None, None, None) != 0


@pytest.mark.parametrize("bad", [None, 5, "val", b"val"])
def test_evaluate_predict_rejects_a_malformed_batches_argument(bad):
    model = next(models())
    with pytest.raises(_lib.HydraMPError, match="batches must be"):
        evaluate.predict(model, bad)


def test_label_buffers_are_checked():
    cpu = torch.device("cpu")
    ok = torch.zeros(8, dtype=torch.int64)
    assert engine._label_buffers(ok, [8], False, cpu)[0] is ok
    assert [o.numel() for o in engine._label_buffers((ok, ok[:3]), [8, 3], True, cpu)] == [8, 3]
    for out, rows, pair in ((torch.zeros(8, dtype=torch.int32), [8], False),    # dtype
                            (torch.zeros(7, dtype=torch.int64), [8], False),    # too few rows
                            (torch.zeros(16, dtype=torch.int64)[::2], [8], False),  # not contiguous
                            (torch.zeros(2, 4, dtype=torch.int64), [8], False),  # not a vector
                            (ok, [8, 8], True),                                  # one buffer for two heads
                            ((ok, None), [8, 8], True),
                            (ok.tolist(), [8], False)):                          # not a tensor
        with pytest.raises(_lib.HydraMPError, match="out"):
            engine._label_buffers(out, rows, pair, cpu)
    with pytest.raises(_lib.HydraMPError, match="out"):
        engine._label_buffers(ok, [8], False, torch.device("meta"))  # another device
