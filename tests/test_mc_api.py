"""CPU checks of the Monte-Carlo dropout interface: the eight new C entries are exported and bound with their argument types, the
ABI is still 4 and no public struct was added or changed size, the Python surface exists on every model class and on both jobs,
nothing runs without a device (there is no CPU fallback), and `samples`, `first_step` and malformed `out` buffers are refused by name
before the device is touched."""
import ctypes as C

import numpy as np
import pytest
import torch

from hydra_gnn_amd import _lib, engine, evaluate, jobs, ops
from test_predict_api import STRUCT_BYTES, models

VP, I32, U32, U64 = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64
PVP, PI32 = C.POINTER(VP), C.POINTER(I32)

NEW_ENTRIES = {
    "hmp_mc_acc_ld": (I32, [I32]),
    "hmp_mc_accumulate_rows": (C.c_int, [VP, I32, I32, I32, VP, I32, VP, I32, VP]),
    "hmp_mc_finish": (C.c_int, [VP, I32, I32, I32, I32, VP, VP, VP, I32, VP, VP, VP, VP]),
    "hmp_head_tails_mc": (C.c_int, [C.POINTER(_lib.TailDesc), I32, I32, I32, I32, PVP, PI32, VP]),
    "hmp_linear_heads_mc": (C.c_int, [C.POINTER(_lib.LinearHeadsDesc), I32, PVP, PI32, PI32, VP]),
    "hmp_net_mc_rooms": (C.c_int, [VP, C.POINTER(_lib.Batch), VP, VP, U64, U32, I32, VP, I32, VP]),
    "hmp_net_mc2": (C.c_int, [VP, C.POINTER(_lib.Batch), VP, U64, U32, I32, PVP, PI32, VP]),
    "hmp_net_mc_heads": (C.c_int, [VP, C.POINTER(_lib.Batch), VP, PVP, U64, U32, I32, PVP, PI32, VP]),
}


def test_new_entries_are_exported_and_bound():
    lib = _lib.load()
    for name, (restype, argtypes) in NEW_ENTRIES.items():
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert name in _lib.SIGNATURES, name
        assert _lib.SIGNATURES[name][0] is restype and list(_lib.SIGNATURES[name][1]) == argtypes, name
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_abi_and_structs_are_unchanged():
    lib = _lib.load()
    assert lib.hmp_abi_version() == 4
    assert [st.__name__ for st in _lib._STRUCTS] == list(STRUCT_BYTES)
    for i, st in enumerate(_lib._STRUCTS):
        assert lib.hmp_sizeof(i) == STRUCT_BYTES[st.__name__] == C.sizeof(st), st.__name__


def test_python_surface_exists():
    assert callable(engine.NativeNet.predict_mc) and callable(engine.NativeNet.predict_uncertainty)
    assert callable(evaluate.predict_mc) and callable(ops.mc_accumulate_rows) and callable(ops.mc_finish) and callable(ops.mc_acc)
    assert callable(jobs.BaseTrainingJob.predict_mc) and callable(jobs.SemiSupervisedTrainingJob.predict_mc)
    for model in models():
        cls = type(model)
        assert callable(getattr(cls, "predict_mc", None)) and callable(getattr(cls, "predict_with_uncertainty", None)), cls.__name__


@pytest.mark.parametrize("C_", [1, 2, 3, 4, 5, 15, 16, 17, 26, 41, 64, 65, 130, 256])
def test_the_accumulator_pitch_holds_the_layout(C_):
    """A at [0, C), B at [Cp, Cp + C), E at 2 Cp with Cp = C rounded up to 4 (include/hydra_mp.h): the pitch covers 2 C + 1 floats and
    keeps rows 16-byte aligned"""
    ld = _lib.load().hmp_mc_acc_ld(C_)
    cp = (C_ + 3) & ~3
    assert ld >= 2 * C_ + 1 and ld > 2 * cp and ld % 4 == 0
    assert _lib.load().hmp_mc_acc_ld(0) == 0 and _lib.load().hmp_mc_acc_ld(-3) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a box WITHOUT a GPU")
@pytest.mark.parametrize("i", range(7))
def test_models_refuse_without_a_device(i):
    model = list(models())[i]
    before = (model._rng_step, model.training)
    with pytest.raises(_lib.HydraMPError, match="no CPU fallback"):
        model.predict_mc(None, samples=3)
    with pytest.raises(_lib.HydraMPError, match="no CPU fallback"):
        model.predict_with_uncertainty(None)
    assert (model._rng_step, model.training) == before


def test_operators_have_no_cpu_path():
    with pytest.raises(_lib.HydraMPError, match="no CPU fallback"):
        ops.mc_accumulate_rows(torch.zeros(3, 4), torch.zeros(3, 12), True)
    with pytest.raises(_lib.HydraMPError, match="no CPU fallback"):
        ops.mc_finish(torch.zeros(3, 12), 4, 2)


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a box WITHOUT a GPU")
def test_entry_points_refuse_without_a_device():
    lib = _lib.load()
    assert lib.hmp_mc_accumulate_rows(None, 4, 3, 4, None, 1, None, 12, None) != 0
    assert lib.hmp_mc_finish(None, 12, 3, 4, 2, None, None, None, 4, None, None, None, None) != 0
    assert lib.hmp_net_mc_rooms(None, None, None, None, 1, 1, 1, None, 12, None) != 0
    acc, ld = (VP * 2)(None, None), (I32 * 2)(12, 12)
    assert lib.hmp_net_mc2(None, None, None, 1, 1, 1, acc, ld, None) != 0
    assert lib.hmp_net_mc_heads(None, None, None, acc, 1, 1, 1, acc, ld, None) != 0
    d = (_lib.TailDesc * 1)()
    assert lib.hmp_head_tails_mc(d, 1, 0, 0, 1, (VP * 1)(None), (I32 * 1)(12), None) != 0 and b"no gfx950 device" in lib.hmp_last_error()
    hd = _lib.LinearHeadsDesc()
    assert lib.hmp_linear_heads_mc(C.byref(hd), 1, acc, ld, None, None) != 0 and b"no gfx950 device" in lib.hmp_last_error()


def test_no_rows_launch_nothing_and_the_ranges_are_checked_first():
    lib = _lib.load()
    assert lib.hmp_mc_accumulate_rows(None, 4, 0, 4, None, 1, None, 12, None) == 0  # no rows: no launch, whatever the device
    for T in (1, 16, 4096):
        assert lib.hmp_mc_finish(None, 12, 0, 4, T, None, None, None, 4, None, None, None, None) == 0
    for T in (0, 4097, -1):
        assert lib.hmp_mc_finish(None, 12, 0, 4, T, None, None, None, 4, None, None, None, None) == 1  # HMP_E_ARG
        assert b"samples = " in lib.hmp_last_error()
    assert lib.hmp_mc_accumulate_rows(None, 4, 0, 4, None, 1, None, 8, None) == 1 and b"ld_acc" in lib.hmp_last_error()
    assert lib.hmp_mc_finish(None, 8, 0, 4, 2, None, None, None, 4, None, None, None, None) == 1 and b"ld_acc" in lib.hmp_last_error()
    assert lib.hmp_mc_finish(None, 12, 0, 4, 2, None, None, None, 3, None, None, None, None) == 0  # no mean: its pitch is not looked at
    buf = (C.c_float * 64)()
    assert lib.hmp_mc_finish(None, 12, 0, 4, 2, None, None, C.addressof(buf), 3, None, None, None, None) == 1 and b"ld_mean" in lib.hmp_last_error()


@pytest.mark.parametrize("samples", [0, 4097, -1, 2.0, None, True, "16"])
def test_samples_outside_1_to_4096_are_refused(samples):
    with pytest.raises(_lib.HydraMPError, match="samples must be"):
        engine._check_samples(samples)
    with pytest.raises(_lib.HydraMPError, match="samples must be"):
        ops.mc_finish(torch.zeros(3, 12), 4, samples)
    with pytest.raises(_lib.HydraMPError, match="samples must be"):
        evaluate.predict_mc(next(models()), [], samples)
    for model in models():
        with pytest.raises(_lib.HydraMPError, match="samples must be"):
            model.predict_mc(None, samples=samples)
        with pytest.raises(_lib.HydraMPError, match="samples must be"):
            model.predict_with_uncertainty(None, samples=samples)


def test_samples_inside_1_to_4096_are_taken():
    assert [engine._check_samples(t) for t in (1, 2, 16, 4096)] == [1, 2, 16, 4096]


@pytest.mark.parametrize("first_step,samples", [(-1, 1), (2 ** 32, 1), (2 ** 32 - 1, 2), (2 ** 32 - 4095, 4096), (1.0, 4), (None, 4), (True, 4)])
def test_first_step_outside_its_range_is_refused(first_step, samples):
    with pytest.raises(_lib.HydraMPError, match="first_step must be"):
        engine._check_first_step(first_step, samples)
    with pytest.raises(_lib.HydraMPError, match="first_step must be"):
        evaluate.predict_mc(next(models()), [], samples, first_step=first_step)
    for model in models():
        with pytest.raises(_lib.HydraMPError, match="first_step must be"):
            model.predict_mc(None, samples=samples, first_step=first_step)


def test_first_step_inside_its_range_is_taken():
    assert engine._check_first_step(0, 1) == 0 and engine._check_first_step(2 ** 32 - 1, 1) == 2 ** 32 - 1
    assert engine._check_first_step(2 ** 32 - 4096, 4096) == 2 ** 32 - 4096 and engine._check_first_step(1, 16) == 1


@pytest.mark.parametrize("seed", [-1, 2 ** 64, 1.5, "7", True])
def test_a_seed_outside_64_bits_is_refused(seed):
    with pytest.raises(_lib.HydraMPError, match="seed must be"):
        engine._check_seed(seed)
    for model in models():
        with pytest.raises(_lib.HydraMPError, match="seed must be"):
            model.predict_mc(None, samples=2, seed=seed)


@pytest.mark.parametrize("bad", [None, 5, "val", b"val"])
def test_evaluate_predict_mc_rejects_a_malformed_batches_argument(bad):
    with pytest.raises(_lib.HydraMPError, match="predict_mc: batches must be"):
        evaluate.predict_mc(next(models()), bad, 3)


def test_evaluate_predict_mc_of_no_batches_is_empty():
    assert evaluate.predict_mc(next(models()), [], 3) == []


def _bufs(n, c, rows=None):
    r = n if rows is None else rows
    return (torch.zeros(r, dtype=torch.int64), torch.zeros(r, c), torch.zeros(r), torch.zeros(r), torch.zeros(r))


def test_mc_buffers_are_checked():
    cpu = torch.device("cpu")
    one = _bufs(8, 5)
    got = engine._mc_buffers(one, [8], [5], False, cpu)
    assert all(a is b for a, b in zip(got[0], one))
    got = engine._mc_buffers((one, _bufs(5, 3)), [8, 5], [5, 3], True, cpu)
    assert [tuple(t.shape) for hd in got for t in hd] == [(8,), (8, 5), (8,), (8,), (8,), (5,), (5, 3), (5,), (5,), (5,)]
    fresh = engine._mc_buffers(None, [4, 0], [5, 3], True, cpu)
    assert [[t.dtype for t in hd] for hd in fresh] == [[torch.int64] + [torch.float32] * 4] * 2
    assert fresh[0][1].shape[1] == 5 and fresh[1][1].shape[1] == 3 and fresh[0][0].numel() >= 4 and all(t.is_contiguous() for t in fresh[0])

    def swap(i, t):
        return tuple(t if j == i else a for j, a in enumerate(one))

    for out, rows, classes, pair in ((swap(0, one[0].int()), [8], [5], False),                       # label dtype
                                     (swap(1, one[1].double()), [8], [5], False),                    # float dtype
                                     (swap(3, one[3].double()), [8], [5], False),
                                     (swap(0, one[0][:7]), [8], [5], False),                         # too few rows
                                     (swap(1, one[1][:7]), [8], [5], False),
                                     (swap(4, one[4][:7]), [8], [5], False),
                                     (swap(1, torch.zeros(8, 6)), [8], [5], False),                  # not C columns
                                     (swap(1, torch.zeros(8, 10)[:, ::2]), [8], [5], False),         # not contiguous
                                     (swap(2, torch.zeros(16)[::2]), [8], [5], False),
                                     (swap(1, torch.zeros(8)), [8], [5], False),                     # a vector for the matrix
                                     (swap(2, torch.zeros(8, 1)), [8], [5], False),                  # a matrix for a vector
                                     (one[:4], [8], [5], False),                                     # four outputs
                                     (one[0], [8], [5], False),                                      # one tensor
                                     (swap(2, None), [8], [5], False),
                                     (one, [8, 8], [5, 5], True),                                    # one head's tuple for two heads
                                     ((one, None), [8, 8], [5, 5], True),
                                     (tuple(t.tolist() for t in one), [8], [5], False)):             # not tensors
        with pytest.raises(_lib.HydraMPError, match="out"):
            engine._mc_buffers(out, rows, classes, pair, cpu)
    with pytest.raises(_lib.HydraMPError, match="out"):
        engine._mc_buffers(one, [8], [5], False, torch.device("meta"))  # another device


def test_split_mc_drops_the_rows_outside_a_head_and_splits_by_graph():
    lab = np.array([3, -1, 0, 2, -1, 1], dtype=np.int64)
    mean = np.arange(12, dtype=np.float32).reshape(6, 2)
    vec = [np.arange(6, dtype=np.float32) + 10 * i for i in range(3)]
    got = evaluate._split_mc([lab, mean] + vec, np.array([2, 0, 4]))
    assert [g[0].tolist() for g in got] == [[3], [], [0, 2, 1]]
    assert got[2][1].tolist() == [[4, 5], [6, 7], [10, 11]] and got[0][2].tolist() == [0.0] and got[2][4].tolist() == [22.0, 23.0, 25.0]
    whole = evaluate._split_mc([np.abs(lab), mean] + vec, np.array([6]))
    assert len(whole) == 1 and whole[0][1].shape == (6, 2)
