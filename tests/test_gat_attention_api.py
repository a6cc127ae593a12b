"""CPU checks of the attention export's interface: the two new C entries are declared in the header, exported and bound with their
argument types, the ABI is still 4 and no public struct was added or changed size, the Python surface exists on every model
class, models without attention are refused by name, and nothing runs without a device (there is no CPU fallback)."""
import ctypes as C
import os
import re

import pytest
import torch

from hydra_gnn_amd import _lib, data, engine
from hydra_gnn_amd.models import (HeterogeneousNetwork, HeterogeneousNeuralTreeNetwork, HomogeneousNetwork,
                                  HomogeneousNeuralTreeNetwork)
from test_predict_api import STRUCT_BYTES, models

VP, I32 = C.c_void_p, C.c_int32
PVP = C.POINTER(VP)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hydra_mp.h")

NEW_ENTRIES = {
    "hmp_gat_attention": [VP, I32, VP, I32, VP, VP, VP, _lib.Plan, _lib.GatArgs, VP, VP, VP, I32, VP, VP, VP],
    "hmp_net_attention": [VP, C.POINTER(_lib.Batch), VP, I32, PVP, I32, PVP, PVP, VP],
}
GAT = dict(GAT_hidden_dims=[8], GAT_heads=[2, 2], GAT_concats=[True, False])
HT_DIMS = {"object": 306, "room": 6, "object-room": 6, "room-room": 6, "object_virtual": 306, "room_virtual": 6}


def gat_models():
    yield HeterogeneousNetwork({"objects": 306, "rooms": 6}, output_dim=26, conv_block="GAT", **GAT)
    yield HeterogeneousNeuralTreeNetwork(HT_DIMS, output_dim=26, conv_block="GAT_edge", **GAT)
    yield HomogeneousNetwork(6, output_dim=26, conv_block="GAT", **GAT)
    yield HomogeneousNeuralTreeNetwork(6, output_dim=26, conv_block="GAT_edge", **GAT)


def test_new_entries_are_declared_exported_and_bound():
    lib = _lib.load()
    header = open(HEADER).read()
    for name, argtypes in NEW_ENTRIES.items():
        assert re.search(r"^int %s\(" % name, header, re.M), f"{name} is not declared in include/hydra_mp.h"
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert name in _lib.SIGNATURES, name
        assert _lib.SIGNATURES[name][0] is C.c_int and list(_lib.SIGNATURES[name][1]) == argtypes, name
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name


def test_abi_and_structs_are_unchanged():
    lib = _lib.load()
    assert lib.hmp_abi_version() == 4 == _lib.ABI_VERSION and _lib.N_KCLASS == 14
    assert re.search(r"^#define HMP_ABI_VERSION 4$", open(HEADER).read(), re.M)
    assert [st.__name__ for st in _lib._STRUCTS] == list(STRUCT_BYTES)
    for i, st in enumerate(_lib._STRUCTS):
        assert lib.hmp_sizeof(i) == STRUCT_BYTES[st.__name__] == C.sizeof(st), st.__name__


def test_python_surface_exists():
    for name in ("attention", "top_attended", "explain", "attention_edge_types", "attention_rows"):
        assert callable(getattr(engine.NativeNet, name, None)), name
    assert callable(data.attention_edge_index)
    for cls in (HeterogeneousNetwork, HeterogeneousNeuralTreeNetwork, HomogeneousNetwork, HomogeneousNeuralTreeNetwork):
        assert callable(getattr(cls, "attention", None)) and callable(getattr(cls, "top_attended", None)), cls.__name__
    assert callable(HeterogeneousNetwork.explain_rooms)


def test_attention_edge_index_appends_the_loops():
    ei = torch.tensor([[0, 2, 2], [1, 1, 2]])
    assert data.attention_edge_index(ei, 3).tolist() == [[0, 2, 2, 0, 1, 2], [1, 1, 2, 0, 1, 2]]
    assert torch.equal(data.attention_edge_index(ei, 0), ei)


@pytest.mark.parametrize("i", range(7))
def test_models_without_attention_are_refused_by_name(i):
    model = list(models())[i]  # GraphSAGE and GCN models
    for call in (lambda: model.attention(None), lambda: model.top_attended(None, k=2)):
        with pytest.raises(_lib.HydraMPError, match=f"no attention coefficients: conv_block {model.conv_block}"):
            call()
    if isinstance(model, HeterogeneousNetwork):
        with pytest.raises(_lib.HydraMPError, match="no attention coefficients: conv_block GraphSAGE"):
            model.explain_rooms(None)


def test_layers_and_inactive_convs_are_refused_by_name():
    het, htree, hom, hom_htree = gat_models()
    for model, bad in ((het, 2), (het, -3), (het, "pre_mp"), (hom, True), (hom, 1.0), (htree, 5)):
        with pytest.raises(_lib.HydraMPError, match="layer|pre_mp"):
            model.attention(None, layer=bad)
    assert htree._attention_layer("pre_mp", "t") == 0 and htree._attention_layer(0, "t") == 1 and htree._attention_layer(-1, "t") == 2
    assert hom_htree._attention_layer("pre_mp", "t") == 0 and hom._attention_layer(-1, "t") == 1
    net = het.native()
    # the room task reads the rooms alone: the last layer's convs into the objects never reach the output
    dead = [c.edge_type for c in net.layers[-1].convs if not c.active]
    assert dead and all(e[2] == "objects" for e in dead)
    assert net.attention_edge_types(1) == [c.edge_type for c in net.layers[1].convs if c.active]
    for call in (lambda: net.attention(None, 1, edge_types=[dead[0]]), lambda: net.top_attended(None, 1, dead[0], 3)):
        with pytest.raises(_lib.HydraMPError, match=re.escape(str(dead[0])) + ".*layer 1.*inactive"):
            call()
    with pytest.raises(_lib.HydraMPError, match="no conv on edge type"):
        net.top_attended(None, 0, ("rooms", "nope", "rooms"), 3)
    with pytest.raises(_lib.HydraMPError, match="out of range"):
        net.attention(None, 2)
    with pytest.raises(_lib.HydraMPError, match="k must be"):
        net.top_attended(None, 1, net.attention_edge_types(1)[0], 9)
    sage = next(models()).native()
    with pytest.raises(_lib.HydraMPError, match="not a GAT layer"):
        sage.attention(None, 0)


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a box WITHOUT a GPU")
@pytest.mark.parametrize("i", range(4))
def test_models_refuse_without_a_device(i):
    model = list(gat_models())[i]
    with pytest.raises(_lib.HydraMPError, match="no CPU fallback"):
        model.attention(None)
    with pytest.raises(_lib.HydraMPError, match="no CPU fallback"):
        model.top_attended(None, k=3)
    if i == 0:
        with pytest.raises(_lib.HydraMPError, match="no CPU fallback"):
            model.explain_rooms(None)


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a box WITHOUT a GPU")
def test_entry_points_refuse_without_a_device():
    lib = _lib.load()
    z = (C.c_float * 64)()
    a = C.addressof(z)
    rc = lib.hmp_gat_attention(a, 8, a, 8, None, None, None, _lib.Plan(), _lib.GatArgs(2, 8, 0, 0, 0.0, 0, 0, 0), a, a, a, 3, None, None, None)
    assert rc != 0 and b"no gfx950 device" in lib.hmp_last_error()
    assert lib.hmp_net_attention(None, None, None, 0, None, 3, None, None, None) != 0


def test_k_is_checked_before_anything_runs():
    lib = _lib.load()
    z = (C.c_float * 64)()
    a = C.addressof(z)
    for k in (0, 9, -1):
        rc = lib.hmp_gat_attention(a, 8, a, 8, None, None, None, _lib.Plan(), _lib.GatArgs(2, 8, 0, 0, 0.0, 0, 0, 0), a, a, a, k, None, None, None)
        assert rc == 1 and b"k = " in lib.hmp_last_error()


def test_attention_buffers_are_checked():
    cpu = torch.device("cpu")
    buf = torch.zeros(8, 2)
    assert engine._attention_buffer(buf, 8, 2, torch.float32, cpu, "out") is buf
    assert engine._attention_buffer(buf, 5, 2, torch.float32, cpu, "out") is buf
    fresh = engine._attention_buffer(None, 0, 3, torch.int64, cpu, "out")
    assert fresh.dtype == torch.int64 and fresh.size(1) == 3 and fresh.is_contiguous()
    for bad in (buf.double(), buf[:7], torch.zeros(8, 3), torch.zeros(8, 4)[:, ::2], buf[:, 0], None.__class__, [buf]):
        with pytest.raises(_lib.HydraMPError, match="out"):
            engine._attention_buffer(bad, 8, 2, torch.float32, cpu, "out")
    with pytest.raises(_lib.HydraMPError, match="out"):
        engine._attention_buffer(buf, 8, 2, torch.float32, torch.device("meta"), "out")
