"""CPU checks of the top-k interface: the six new C entries are exported and bound with their argument types, the ABI is still 4
and no public struct was added or changed size, the Python surface exists on every model class, nothing runs without a device
(there is no CPU fallback), k outside [1, 8] and malformed `out` buffers are refused before the device is touched."""
import ctypes as C

import pytest
import torch

from hydra_gnn_amd import _lib, engine, evaluate, jobs, ops
from test_predict_api import STRUCT_BYTES, models

VP, I32 = C.c_void_p, C.c_int32
PVP = C.POINTER(VP)

NEW_ENTRIES = {
    "hmp_topk_rows": [VP, I32, I32, I32, VP, I32, VP, VP, VP],
    "hmp_head_tails_topk": [C.POINTER(_lib.TailDesc), I32, I32, I32, I32, PVP, PVP, VP],
    "hmp_linear_heads_topk": [C.POINTER(_lib.LinearHeadsDesc), I32, PVP, PVP, C.POINTER(I32), VP],
    "hmp_net_topk_rooms": [VP, C.POINTER(_lib.Batch), VP, VP, I32, VP, VP, VP],
    "hmp_net_topk2": [VP, C.POINTER(_lib.Batch), VP, I32, PVP, PVP, VP],
    "hmp_net_topk_heads": [VP, C.POINTER(_lib.Batch), VP, PVP, I32, PVP, PVP, VP],
}


def test_new_entries_are_exported_and_bound():
    lib = _lib.load()
    for name, argtypes in NEW_ENTRIES.items():
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert name in _lib.SIGNATURES, name
        assert _lib.SIGNATURES[name][0] is C.c_int and list(_lib.SIGNATURES[name][1]) == argtypes, name
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name


def test_abi_and_structs_are_unchanged():
    lib = _lib.load()
    assert lib.hmp_abi_version() == 4
    assert [st.__name__ for st in _lib._STRUCTS] == list(STRUCT_BYTES)
    for i, st in enumerate(_lib._STRUCTS):
        assert lib.hmp_sizeof(i) == STRUCT_BYTES[st.__name__] == C.sizeof(st), st.__name__


def test_python_surface_exists():
    assert callable(engine.NativeNet.predict_topk) and callable(engine.NativeNet.predict_confidence)
    assert callable(evaluate.predict_topk) and callable(ops.topk_rows)
    assert callable(jobs.BaseTrainingJob.predict_topk) and callable(jobs.SemiSupervisedTrainingJob.predict_topk)
    for model in models():
        cls = type(model)
        assert callable(getattr(cls, "predict_topk", None)) and callable(getattr(cls, "predict_with_confidence", None)), cls.__name__


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a box WITHOUT a GPU")
@pytest.mark.parametrize("i", range(7))
def test_models_refuse_without_a_device(i):
    model = list(models())[i]
    with pytest.raises(_lib.HydraMPError, match="no CPU fallback"):
        model.predict_topk(None, k=3)
    with pytest.raises(_lib.HydraMPError, match="no CPU fallback"):
        model.predict_with_confidence(None)


def test_operator_has_no_cpu_path():
    with pytest.raises(_lib.HydraMPError, match="no CPU fallback"):
        ops.topk_rows(torch.zeros(3, 4), 2)


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a box WITHOUT a GPU")
def test_entry_points_refuse_without_a_device():
    lib = _lib.load()
    assert lib.hmp_topk_rows(None, 4, 3, 4, None, 2, None, None, None) != 0
    assert lib.hmp_net_topk_rooms(None, None, None, None, 2, None, None, None) != 0
    assert lib.hmp_net_topk2(None, None, None, 2, None, None, None) != 0
    assert lib.hmp_net_topk_heads(None, None, None, None, 2, None, None, None) != 0
    d = (_lib.TailDesc * 1)()
    out = (VP * 1)(None)
    assert lib.hmp_head_tails_topk(d, 1, 0, 0, 2, out, out, None) != 0 and b"no gfx950 device" in lib.hmp_last_error()
    hd = _lib.LinearHeadsDesc()
    out2 = (VP * 2)(None, None)
    assert lib.hmp_linear_heads_topk(C.byref(hd), 2, out2, out2, None, None) != 0 and b"no gfx950 device" in lib.hmp_last_error()


def test_no_rows_launch_nothing_and_k_is_checked_first():
    lib = _lib.load()
    for k in range(1, 9):
        assert lib.hmp_topk_rows(None, 4, 0, 4, None, k, None, None, None) == 0  # no rows: no launch, whatever the device
    for k in (0, 9, -1):
        assert lib.hmp_topk_rows(None, 4, 0, 4, None, k, None, None, None) == 1  # HMP_E_ARG
        assert b"k = " in lib.hmp_last_error()


@pytest.mark.parametrize("k", [0, 9, -1, 2.0, None, True])
def test_k_outside_1_to_8_is_refused(k):
    with pytest.raises(_lib.HydraMPError, match="k must be"):
        engine._check_k(k)
    with pytest.raises(_lib.HydraMPError, match="k must be"):
        ops.topk_rows(torch.zeros(3, 4), k)
    with pytest.raises(_lib.HydraMPError, match="k must be"):
        evaluate.predict_topk(next(models()), [], k)


def test_k_inside_1_to_8_is_taken():
    assert [engine._check_k(k) for k in range(1, 9)] == list(range(1, 9))


@pytest.mark.parametrize("bad", [None, 5, "val", b"val"])
def test_evaluate_predict_topk_rejects_a_malformed_batches_argument(bad):
    with pytest.raises(_lib.HydraMPError, match="predict_topk: batches must be"):
        evaluate.predict_topk(next(models()), bad, 3)


def test_topk_buffers_are_checked():
    cpu = torch.device("cpu")
    lab, prb = torch.zeros(8, 3, dtype=torch.int64), torch.zeros(8, 3)
    got = engine._topk_buffers((lab, prb), [8], 3, False, cpu)
    assert got[0][0] is lab and got[0][1] is prb
    got = engine._topk_buffers(((lab, prb), (lab[:5], prb[:5])), [8, 5], 3, True, cpu)
    assert [tuple(t.shape) for pair in got for t in pair] == [(8, 3), (8, 3), (5, 3), (5, 3)]
    fresh = engine._topk_buffers(None, [4, 0], 2, True, cpu)
    assert [(p[0].dtype, p[1].dtype, p[0].size(1), p[1].size(1)) for p in fresh] == [(torch.int64, torch.float32, 2, 2)] * 2
    assert fresh[0][0].size(0) >= 4 and fresh[0][0].is_contiguous() and fresh[0][1].is_contiguous()
    for out, rows, pair in (((lab.int(), prb), [8], False),                                  # label dtype
                            ((lab, prb.double()), [8], False),                               # probability dtype
                            ((lab[:7], prb), [8], False),                                    # too few rows
                            ((lab, prb[:7]), [8], False),
                            ((torch.zeros(8, 4, dtype=torch.int64), prb), [8], False),       # not k columns
                            ((lab, torch.zeros(8, 2)), [8], False),
                            ((torch.zeros(8, 6, dtype=torch.int64)[:, ::2], prb), [8], False),  # not contiguous
                            ((lab, torch.zeros(16, 3)[::2]), [8], False),
                            ((lab[:, 0], prb[:, 0]), [8], False),                            # vectors
                            (lab, [8], False),                                               # one tensor, no pair
                            ((lab, None), [8], False),
                            ((lab, prb), [8, 8], True),                                      # one head's pair for two heads
                            (((lab, prb), None), [8, 8], True),
                            ((lab.tolist(), prb.tolist()), [8], False)):                     # not tensors
        with pytest.raises(_lib.HydraMPError, match="out"):
            engine._topk_buffers(out, rows, 3, pair, cpu)
    with pytest.raises(_lib.HydraMPError, match="out"):
        engine._topk_buffers((lab, prb), [8], 3, False, torch.device("meta"))  # another device
