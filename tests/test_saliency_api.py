"""CPU checks of the gradient-saliency interface: the new C entries are declared in the header, exported and bound with their
argument types, the ABI is still 4 and no public struct was added or changed size; the Python surface exists on every model class;
arguments are checked and unsupported models refused by name before anything needs a device; nothing runs without one; and the
float64 / exact reference helpers of tests/_saliency_reference.py agree with hand-written cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from hydra_gnn_amd import _lib, engine, evaluate, jobs
from hydra_gnn_amd.models import (HeterogeneousNetwork, HeterogeneousNeuralTreeNetwork, HomogeneousNetwork,
                                  HomogeneousNeuralTreeNetwork)
from test_predict_api import STRUCT_BYTES, models
from _saliency_reference import (SEL_MASK, SEL_ORDINAL, WRT_LOGPROB, first_argmax, scores_reference, seed_reference, selected_rows,
                                 top_from_scores)

VP, I32 = C.c_void_p, C.c_int32
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hydra_mp.h")
NEW_ENTRIES = {
    "hmp_saliency_seed": [VP, I32, I32, I32, VP, I32, VP, I32, VP, I32, I32, VP, I32, VP],
    "hmp_saliency_scores": [VP, I32, VP, I32, I32, I32, I32, C.POINTER(I32), C.POINTER(I32), VP, VP, VP, VP],
    "hmp_saliency_topk": [_lib.Plan, VP, I32, I32, VP, I32, VP, I32, VP, VP, VP],
    "hmp_net_input_gradient": [VP, C.POINTER(_lib.Batch), VP, I32, VP, I32, VP, I32, VP, I32, I32, C.POINTER(VP), VP],
    "hmp_net_plan": [VP, I32, C.POINTER(_lib.Plan)],
}
HT_DIMS = {"object": 306, "room": 6, "object-room": 6, "room-room": 6, "object_virtual": 306, "room_virtual": 6}
SAGE = dict(conv_block="GraphSAGE", hidden_dim=8, num_layers=2)


def test_new_entries_are_declared_exported_and_bound():
    lib = _lib.load()
    header = open(HEADER).read()
    for name, argtypes in NEW_ENTRIES.items():
        assert re.search(r"^int %s\(" % name, header, re.M), f"{name} is not declared in include/hydra_mp.h"
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert _lib.SIGNATURES[name][0] is C.c_int and list(_lib.SIGNATURES[name][1]) == argtypes, name
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name
    for macro, value in (("HMP_SEL_ALL", 0), ("HMP_SEL_MASK", 1), ("HMP_SEL_ORDINAL", 2), ("HMP_WRT_LOGIT", 0), ("HMP_WRT_LOGPROB", 1)):
        assert re.search(r"^#define %s %d$" % (macro, value), header, re.M), macro
    assert (engine.SEL_ALL, engine.SEL_MASK, engine.SEL_ORDINAL) == (0, 1, 2) and engine.WRT_CODES == {"logit": 0, "logprob": 1}


def test_abi_and_structs_are_unchanged():
    lib = _lib.load()
    assert lib.hmp_abi_version() == 4 == _lib.ABI_VERSION
    assert [st.__name__ for st in _lib._STRUCTS] == list(STRUCT_BYTES)
    for i, st in enumerate(_lib._STRUCTS):
        assert lib.hmp_sizeof(i) == STRUCT_BYTES[st.__name__] == C.sizeof(st), st.__name__


def test_python_surface_exists():
    for name in ("input_gradients", "saliency", "top_salient", "explain_salient", "saliency_scores", "salient_edge_types", "max_graph_rows"):
        assert callable(getattr(engine.NativeNet, name, None)), name
    for cls in (HeterogeneousNetwork, HeterogeneousNeuralTreeNetwork, HomogeneousNetwork, HomogeneousNeuralTreeNetwork):
        for name in ("input_gradients", "saliency", "top_salient"):
            assert callable(getattr(cls, name, None)), (cls.__name__, name)
    for cls in (HeterogeneousNetwork, HeterogeneousNeuralTreeNetwork, HomogeneousNetwork, HomogeneousNeuralTreeNetwork):
        assert callable(getattr(cls, "explain_rooms", None)), cls.__name__
    assert callable(evaluate.saliency) and callable(jobs.BaseTrainingJob.saliency)


def sage_net():
    return HeterogeneousNetwork({"objects": 306, "rooms": 6}, output_dim=26, **SAGE).native()


def test_arguments_are_checked_before_a_device_is_needed():
    net = sage_net()
    for k in (0, 9, -1, True, 2.0):
        with pytest.raises(_lib.HydraMPError, match="k must be"):
            net.top_salient(None, ("objects", "objects_to_rooms", "rooms"), k)
    for wrt in ("prob", 0, None):
        with pytest.raises(_lib.HydraMPError, match="wrt must be"):
            net.input_gradients(None, wrt=wrt)
    with pytest.raises(_lib.HydraMPError, match="column groups"):
        net.saliency(None, groups=((0, 1), (1, 2), (2, 3), (3, 4), (4, 5)))
    with pytest.raises(_lib.HydraMPError, match=r"\(lo, hi\)"):
        net.saliency(None, groups=(3,))
    rows = torch.ones(3, dtype=torch.bool)
    for call in (lambda: net.input_gradients(None, rows=rows, ordinal=0), lambda: net.saliency(None, rows=rows, ordinal=(0, rows))):
        with pytest.raises(_lib.HydraMPError, match="rows and ordinal overlap"):
            call()
    with pytest.raises(_lib.HydraMPError, match="passes and rows / ordinal overlap"):
        net.top_salient(None, ("objects", "objects_to_rooms", "rooms"), 3, passes=2, rows=rows)
    for bad in (-1, 1.5, True, ("a", None)):
        with pytest.raises(_lib.HydraMPError, match="ordinal must be"):
            net.input_gradients(None, ordinal=bad)
    with pytest.raises(_lib.HydraMPError, match="head 1"):
        net.input_gradients(None, head=1)
    with pytest.raises(_lib.HydraMPError, match="no edge type"):
        net.top_salient(None, ("rooms", "nope", "rooms"), 3)
    with pytest.raises(_lib.HydraMPError, match="does not end in 'rooms'"):
        net.top_salient(None, ("rooms", "rooms_to_objects", "objects"), 3, passes=1)
    assert net._score_ranges(((0, 3), (3, 6), (6, None), (300, 400)), 306, "t") == ([0, 3, 6, 300], [3, 6, 306, 306])
    assert net.head_type(0) == "rooms" and set(net.salient_edge_types()) <= set(net.edge_types)
    het = HeterogeneousNetwork({"objects": 306, "rooms": 6}, output_dim=26, **SAGE)
    with pytest.raises(_lib.HydraMPError, match="by must be"):
        het.explain_rooms(None, by="saliency")


def test_models_outside_the_native_program_are_refused_by_name():
    gcn = HomogeneousNetwork(6, output_dim=15, conv_block="GCN", hidden_dim=8, num_layers=2)
    gin = HomogeneousNeuralTreeNetwork(6, output_dim=15, conv_block="GIN", hidden_dim=8, num_layers=2, disable_initialization=True)
    for model, block in ((gcn, "GCN"), (gin, "GIN")):
        for call in (lambda: model.input_gradients(None), lambda: model.saliency(None), lambda: model.top_salient(None)):
            with pytest.raises(_lib.HydraMPError, match=f"{block} models run op by op"):
                call()
    heads = HomogeneousNetwork(6, output_dim_dict={"rooms": 15, "objects": 20}, **SAGE)
    for call in (lambda: heads.input_gradients(None), lambda: heads.saliency(None), lambda: heads.top_salient(None)):
        with pytest.raises(_lib.HydraMPError, match="learned linear heads"):
            call()
    pooled = list(models())[2]  # the two-headed H-tree model: its heads read a LeafPool
    with pytest.raises(_lib.HydraMPError, match="pooled heads"):
        pooled.input_gradients(None)
    bf16 = HeterogeneousNetwork({"objects": 306, "rooms": 6}, output_dim=26, **SAGE)
    bf16.native().set_compute("bf16")
    for call in (lambda: bf16.input_gradients(None), lambda: bf16.explain_rooms(None, by="gradient")):
        with pytest.raises(_lib.HydraMPError, match="bf16 compute mode"):
            call()
    with pytest.raises(_lib.HydraMPError, match="explain_rooms: the model is two-headed"):
        heads.explain_rooms(None)
    with pytest.raises(_lib.HydraMPError, match="GCN models run op by op"):
        gcn.explain_rooms(None)
    two = list(models())[1]
    with pytest.raises(_lib.HydraMPError, match="two-headed"):
        two._explain_by_gradient(None, 3)


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a box WITHOUT a GPU")
def test_models_refuse_without_a_device():
    het = HeterogeneousNetwork({"objects": 306, "rooms": 6}, output_dim=26, **SAGE)
    gat = HeterogeneousNetwork({"objects": 306, "rooms": 6}, output_dim=26, conv_block="GAT", GAT_hidden_dims=[8], GAT_heads=[2, 2],
                               GAT_concats=[True, False])
    htree = HeterogeneousNeuralTreeNetwork(HT_DIMS, output_dim=26, disable_initialization=True, **SAGE)
    hom = HomogeneousNetwork(6, output_dim=15, **SAGE)
    for model in (het, gat, htree, hom):
        for call in (lambda: model.input_gradients(None), lambda: model.saliency(None), lambda: model.top_salient(None)):
            with pytest.raises(_lib.HydraMPError, match="no CPU fallback"):
                call()
    for call in (lambda: het.explain_rooms(None, by="gradient"), lambda: gat.explain_rooms(None, by="gradient"), lambda: htree.explain_rooms(None)):
        with pytest.raises(_lib.HydraMPError, match="no CPU fallback"):
            call()


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a box WITHOUT a GPU")
def test_entry_points_refuse_without_a_device():
    lib = _lib.load()
    z = (C.c_float * 64)()
    a = C.addressof(z)
    assert lib.hmp_saliency_seed(a, 8, 0, 8, None, 0, None, 0, None, 0, 0, a, 8, None) == 0  # no rows: no launch
    assert lib.hmp_saliency_seed(a, 8, 4, 8, None, 0, None, 0, None, 0, 0, a, 8, None) != 0
    assert lib.hmp_saliency_scores(a, 8, a, 8, 4, 8, 0, None, None, a, None, None, None) != 0
    assert lib.hmp_net_input_gradient(None, None, None, 0, None, 0, None, 0, None, 0, 0, None, None) != 0
    assert lib.hmp_net_plan(None, 0, None) != 0


def test_arguments_of_the_unit_entries_are_checked_before_anything_runs():
    lib = _lib.load()
    z = (C.c_float * 64)()
    a = C.addressof(z)
    for k in (0, 9, -1):
        assert lib.hmp_saliency_topk(_lib.Plan(), a, k, 0, None, 0, None, 0, a, a, None) == 1 and b"k = " in lib.hmp_last_error()
    assert lib.hmp_saliency_seed(a, 8, 4, 8, None, 0, None, 0, None, 0, 7, a, 8, None) == 1 and b"wrt" in lib.hmp_last_error()
    assert lib.hmp_saliency_seed(a, 8, 4, 8, None, 9, None, 0, None, 0, 0, a, 8, None) == 1 and b"selection mode" in lib.hmp_last_error()
    assert lib.hmp_saliency_seed(a, 4, 4, 8, None, 0, None, 0, None, 0, 0, a, 8, None) == 1
    lo = (I32 * 5)()
    assert lib.hmp_saliency_scores(a, 8, a, 8, 4, 8, 5, lo, lo, a, None, None, None) == 1 and b"column ranges" in lib.hmp_last_error()


# ---- the reference helpers against hand-written cases ------------------------------------------------------------------------------
def test_selected_rows_by_hand():
    ptr = [0, 2, 2, 5, 6]  # graphs of 2, 0, 3 and 1 rows
    assert selected_rows(6, SEL_ORDINAL, p=0, ptr=ptr).tolist() == [True, False, True, False, False, True]
    assert selected_rows(6, SEL_ORDINAL, p=1, ptr=ptr).tolist() == [False, True, False, True, False, False]
    assert selected_rows(6, SEL_ORDINAL, p=2, ptr=ptr).tolist() == [False, False, False, False, True, False]
    assert not selected_rows(6, SEL_ORDINAL, p=3, ptr=ptr).any()
    assert selected_rows(3, SEL_MASK, mask=[1, 0, 2]).tolist() == [True, False, True] and selected_rows(2).all()
    total = sum(selected_rows(6, SEL_ORDINAL, p=p, ptr=ptr).astype(int) for p in range(3))
    assert total.tolist() == [1] * 6  # the ordinals partition the rows


def test_seed_reference_by_hand():
    z = np.array([[0.0, 2.0, 2.0, 9.0], [1.0, 1.0, 1.0, 9.0], [np.log(1.0), np.log(3.0), np.log(4.0), 9.0]], dtype=np.float32)
    assert first_argmax(z[:, :3]).tolist() == [1, 0, 2]  # the first maximum; column 3 is padding
    out, cls = seed_reference(z, 3, 5)
    assert cls.tolist() == [1, 0, 2] and out.tolist() == [[0, 1, 0, 0, 0], [1, 0, 0, 0, 0], [0, 0, 1, 0, 0]]
    out, cls = seed_reference(z, 3, 4, target=[0, -1, 3], sel=[True, True, False])
    assert cls.tolist() == [0, 0, 2] and out.tolist() == [[1, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]]  # out-of-range targets: the prediction
    out, _ = seed_reference(z, 3, 4, wrt=WRT_LOGPROB)
    np.testing.assert_allclose(out[2], [-1 / 8, -3 / 8, 1 - 4 / 8, 0], atol=1e-7)  # log(1), log(3), log(4): softmax 1/8, 3/8, 4/8
    np.testing.assert_allclose(out[1], [1 - 1 / 3, -1 / 3, -1 / 3, 0], atol=1e-12)
    np.testing.assert_allclose(out.sum(axis=1), 0, atol=1e-7)


def test_scores_reference_by_hand():
    g = np.array([[1.0, -2.0, 3.0, 100.0], [0.0, 0.0, 0.0, 100.0]])
    x = np.array([[2.0, 1.0, -1.0, 100.0], [5.0, 5.0, 5.0, 100.0]])
    gxi, gnorm, grp, scale = scores_reference(g, x, 3, ((0, 1), (1, None), (2, 9), (2, 2), (5, 3)))
    assert gxi.tolist() == [-3.0, 0.0] and scale.tolist() == [7.0, 0.0]
    np.testing.assert_allclose(gnorm, [np.sqrt(14.0), 0.0])
    assert grp.tolist() == [[2.0, -5.0, -3.0, 0.0, 0.0], [0.0] * 5]
    assert scores_reference(g, x, 3)[2].shape == (2, 0)


def test_top_from_scores_by_hand():
    score = np.array([0.5, -2.0, 2.0, 0.0, -0.5], dtype=np.float32)
    #        destination 0: sources 0, 1, 2, 2 (a duplicate), 4;  destination 1: none;  destination 2: source 3;  one edge out of range
    ei = np.array([[0, 1, 2, 2, 4, 3, 7], [0, 0, 0, 0, 0, 2, 0]])
    src, sc = top_from_scores(score, ei, 5, 3, 3)
    assert src.tolist() == [[1, 2, 0], [-1, -1, -1], [3, -1, -1]]  # |-2| == |2|: the lower source first; 0.5 before -0.5 likewise
    assert sc.tolist() == [[-2.0, 2.0, 0.5], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    src, sc = top_from_scores(score, ei, 5, 3, 8)
    assert src[0].tolist() == [1, 2, 0, 4, -1, -1, -1, -1] and sc[0, 3] == np.float32(-0.5)  # the duplicate is listed once
    src, sc = top_from_scores(score, ei, 5, 3, 1, sel=[False, True, True])
    assert src.tolist() == [[-7], [-1], [3]] and sc.tolist() == [[-7.0], [0.0], [0.0]]  # unselected rows keep the prefill
