"""Attention export through the executor: model.attention / model.top_attended on all four model classes x GAT / GAT_edge at
their smallest configurations, against the coefficients of the ``oracle.models`` twin (same weights, float64).

The oracle's coefficients are captured by wrapping every oracle GATConv instance's ``forward`` to call itself with
``return_alpha=True``: it hands out (edge_index after remove / add self loops, alpha before dropout).  Its loop-free index is
mapped back to original edge ids: the kept edges are the input edges minus, for a conv with self loops, the input edges i -> i,
in input order; the appended loops follow.  Tolerance 1e-5 (atol + rtol), the project's standing fp32 bound against float64.
Stream descriptors and host batches run the same kernels on the same bytes: bit-equal.  The launch budget is the eval forward's
launches plus exactly one (class gat_fwd)."""
import copy
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from hydra_gnn_amd import _lib, workloads  # noqa: E402
from hydra_gnn_amd.data import attention_edge_index, collate, collate_homogeneous  # noqa: E402
from hydra_gnn_amd.models import (HeterogeneousNetwork, HeterogeneousNeuralTreeNetwork, HomogeneousNetwork,  # noqa: E402
                                  HomogeneousNeuralTreeNetwork)
from hydra_gnn_amd.store import GraphStore  # noqa: E402
from oracle import models as omodels  # noqa: E402
from oracle import pyg_ref  # noqa: E402
from test_gpu_predict_models import launches  # noqa: E402

ATOL, RTOL = 1e-5, 1e-5
DEV = "cuda:0"
KC_GAT_FWD = 9
SHAPES = ("hetero", "hetero_htree", "homog", "homog_htree")
BLOCKS = ("GAT", "GAT_edge")
HT_DIMS = {"object": 306, "room": 6, "object-room": 6, "room-room": 6, "object_virtual": 306, "room_virtual": 6}
CLASS_OF = {"hetero": (HeterogeneousNetwork, omodels.HeterogeneousNetwork),
            "hetero_htree": (HeterogeneousNeuralTreeNetwork, omodels.HeterogeneousNeuralTreeNetwork),
            "homog": (HomogeneousNetwork, omodels.HomogeneousNetwork),
            "homog_htree": (HomogeneousNeuralTreeNetwork, omodels.HomogeneousNeuralTreeNetwork)}


def model_kw(shape, block):
    """the two-headed models (every last-layer conv is live, and store.stream needs no label type), H-trees with their pre_mp"""
    if shape == "hetero":
        dims = {"objects": 306, "rooms": 6} if block == "GAT" else {"objects": 303, "rooms": 3}
        return dict(input_dim_dict=dims, output_dim_dict={"rooms": 26, "objects": 28}, conv_block=block, GAT_hidden_dims=[8],
                    GAT_heads=[2, 2], GAT_concats=[True, False], dropout=0.0)
    if shape == "hetero_htree":
        return dict(input_dim_dict=dict(HT_DIMS), output_dim_dict={"room": 15, "object": 35, "object-room": 1, "room-room": 1},
                    conv_block=block, GAT_hidden_dims=[8], GAT_heads=[2, 2], GAT_concats=[True, False], dropout=0.0)
    return dict(input_dim=6, output_dim_dict={"room": 15, "object": 35}, conv_block=block, GAT_hidden_dims=[8, 8], GAT_heads=[2, 2],
                GAT_concats=[True, False], dropout=0.0)


def graphs_of(shape, block, n, seed):
    edge = block == "GAT_edge"
    if shape == "hetero":
        return workloads.semisupervised_graphs(n, seed, relative_pos=edge)
    if shape == "hetero_htree":
        return workloads.semisupervised_htree_graphs(n, seed, relative_pos=edge)
    if shape == "homog":
        return workloads.stanford_semisupervised_graphs(n, seed, edge_attr=edge)
    return workloads.stanford_htree_semisupervised_graphs(n, seed, edge_attr=edge)


def coll(shape, graphs):
    return collate_homogeneous(graphs) if shape.startswith("homog") else collate(graphs)


def pair_of(shape, block, seed):
    torch.manual_seed(seed)
    kw = model_kw(shape, block)
    cls, ocls = CLASS_OF[shape]
    ora = ocls(**kw)
    with torch.no_grad():  # the oracle's GATConv bias starts at zero
        for name, p in ora.named_parameters():
            if name.endswith("bias"):
                p.uniform_(-0.1, 0.1)
    net = cls(**kw)
    net.load_state_dict(ora.state_dict(), strict=True)
    return ora, net.to(DEV).eval()


def oracle_attention(ora, shape, batch):
    """{(layer | "pre_mp", edge type | None): (edge_index after remove / add self loops, alpha float64, conv adds self loops)}"""
    o64 = copy.deepcopy(ora).double().eval()
    rec = {}
    for name, m in o64.named_modules():
        if not isinstance(m, pyg_ref.GATConv):
            continue
        parts = name.split(".")
        layer = "pre_mp" if parts[0] == "pre_mp" else int(parts[1])
        et = tuple(parts[-1].split("__")) if parts[-2:-1] == ["convs"] and "__" in parts[-1] else None

        def fwd(*a, _orig=m.forward, _key=(layer, et), _loops=bool(m.add_self_loops), **k):
            out, (ei, alpha) = _orig(*a, return_alpha=True, **k)
            rec[_key] = (ei, alpha.detach(), _loops)
            return out

        m.forward = fwd
    if shape.startswith("homog"):
        batch.x = batch.x.double()
        if getattr(batch, "edge_attr", None) is not None:
            batch.edge_attr = batch.edge_attr.double()
    else:
        for t in batch.node_types:
            if "x" in batch[t]:
                batch[t].x = batch[t].x.double()
        for et in batch.edge_types:
            if "edge_attr" in batch[et]:
                batch[et].edge_attr = batch[et].edge_attr.double()
    with torch.no_grad():
        o64(batch)
    return rec


def compare(got, ei, ref, tag):
    """got: exported alpha [E + n_loop, H] (device); ei: the conv's input edge_index (host); ref: the oracle's record"""
    ref_ei, ref_alpha, loops = ref
    E = ei.size(1)
    kept = ei[0] != ei[1] if loops else torch.ones(E, dtype=torch.bool)
    nk = int(kept.sum())
    n_loop = ref_ei.size(1) - nk
    assert n_loop >= 0 and (loops or n_loop == 0), tag
    assert torch.equal(ref_ei[:, :nk], ei[:, kept]), f"{tag}: the oracle's kept edges are not the input edges in input order"
    g = got.cpu()
    assert g.dtype == torch.float32 and tuple(g.shape) == (E + n_loop, ref_alpha.size(1)), f"{tag}: shape {tuple(g.shape)}"
    full = attention_edge_index(ei, n_loop)
    assert torch.equal(full[:, E:], ref_ei[:, nk:]), f"{tag}: the loop rows"
    err = float((g[:E][kept].double() - ref_alpha[:nk]).abs().max()) if nk else 0.0
    print(f"{tag}: E={E} kept={nk} loops={n_loop} max |alpha - oracle| = {err:.3e}")
    torch.testing.assert_close(g[:E][kept].double(), ref_alpha[:nk], atol=ATOL, rtol=RTOL, msg=lambda m: f"{tag} (edges): {m}")
    torch.testing.assert_close(g[E:].double(), ref_alpha[nk:], atol=ATOL, rtol=RTOL, msg=lambda m: f"{tag} (loops): {m}")
    assert bool((g[:E][~kept] == 0).all()), f"{tag}: a removed self loop's row is not 0"


def input_edges(shape, batch, layer, et):
    if shape.startswith("homog"):
        return batch.init_edge_index if layer == "pre_mp" else batch.edge_index
    return batch[et].edge_index


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("shape", SHAPES)
def test_attention_equals_the_oracle(shape, block):
    ora, net = pair_of(shape, block, seed=3 + SHAPES.index(shape))
    gs = graphs_of(shape, block, 3, seed=31 + SHAPES.index(shape))
    host = coll(shape, gs)
    ref = oracle_attention(ora, shape, coll(shape, gs))
    batch = coll(shape, gs).to(DEV)
    nat = net.native()
    layers = list(range(net.num_layers)) + (["pre_mp"] if "htree" in shape else [])
    assert {k[0] for k in ref} == set(layers)
    seen = 0
    for layer in layers:
        got = net.attention(batch, layer=layer)
        if shape.startswith("homog"):
            assert isinstance(got, torch.Tensor) and got.is_cuda
            got = {None: got}
        else:
            prog = nat.layers[net._attention_layer(layer, "test")]
            assert set(got) == {c.edge_type for c in prog.convs if c.active} and len(got) > 0
        for et, alpha in got.items():
            compare(alpha, input_edges(shape, host, layer, et), ref[(layer, et)], f"{shape} {block} layer {layer} {et}")
            seen += 1
        # top_attended is the order of the exported alpha (checked bit for bit at the unit entry): here its shape and column 0
        top = net.top_attended(batch, k=2, layer=layer)
        top = {None: top} if shape.startswith("homog") else top
        assert set(top) == set(got)
        for et, (src, w) in top.items():
            ei = input_edges(shape, host, layer, et)
            n_dst = src.size(0)
            assert src.dtype == torch.int64 and w.dtype == torch.float32 and tuple(src.shape) == tuple(w.shape) == (n_dst, 2)
            mean = got[et].cpu().mean(dim=1)
            full = attention_edge_index(ei, got[et].size(0) - ei.size(1))
            best = torch.full((n_dst,), -1.0).scatter_reduce(0, full[1], mean, "amax", include_self=True)
            has = best >= 0
            torch.testing.assert_close(w[:, 0].cpu()[has], best[has], atol=1e-6, rtol=1e-6)
            assert bool((src[:, 0].cpu()[~has] == -1).all()) and bool((w[:, 0].cpu()[~has] == 0).all())
    # two-headed nets: every conv is live, but for the H-tree's last-layer convs into the clique types (no head reads those)
    assert seen == len(ref) if shape != "hetero_htree" else 0 < seen < len(ref)
    last, dflt = net.attention(batch, layer=net.num_layers - 1), net.attention(batch)  # layer=-1 is the default
    if shape.startswith("homog"):
        last, dflt = {None: last}, {None: dflt}
    assert set(last) == set(dflt) and all(torch.equal(last[e], dflt[e]) for e in last)


@pytest.mark.parametrize("shape", SHAPES)
def test_stream_descriptors_give_the_bits_of_host_batches(shape):
    _, net = pair_of(shape, "GAT", seed=11)
    gs = graphs_of(shape, "GAT", 6, seed=41)
    store = GraphStore(gs, DEV)
    stream = store.stream(net, 4)
    layers = list(range(net.num_layers)) + (["pre_mp"] if "htree" in shape else [])
    for ids in ([0, 1, 2], [5], [4, 4, 3]):
        host = coll(shape, [gs[i] for i in ids]).to(DEV)
        for layer in layers:
            want = net.attention(host, layer=layer)
            want_top = net.top_attended(host, k=3, layer=layer)
            got = net.attention(stream.next(ids), layer=layer)
            got_top = net.top_attended(stream.next(ids), k=3, layer=layer)
            if shape.startswith("homog"):
                want, got, want_top, got_top = {None: want}, {None: got}, {None: want_top}, {None: got_top}
            assert set(want) == set(got) and set(want_top) == set(got_top)
            for et in want:
                assert want[et].numel() > 0 and torch.equal(want[et].view(torch.int32), got[et].view(torch.int32)), (shape, ids, layer, et)
                assert torch.equal(want_top[et][0], got_top[et][0]), (shape, ids, layer, et)
                assert torch.equal(want_top[et][1].view(torch.int32), got_top[et][1].view(torch.int32)), (shape, ids, layer, et)
    other = pair_of(shape, "GAT", seed=11)[1]
    with pytest.raises(_lib.HydraMPError, match="another model"):
        other.attention(stream.next([0, 1]))


def room_model(block="GAT"):
    torch.manual_seed(5)
    dims = {"objects": 306, "rooms": 6} if block == "GAT" else {"objects": 303, "rooms": 3}
    net = HeterogeneousNetwork(input_dim_dict=dims, output_dim=26, conv_block=block, GAT_hidden_dims=[8], GAT_heads=[2, 2],
                               GAT_concats=[True, False], dropout=0.0)
    return net.to(DEV).eval()


def test_an_inactive_conv_is_refused_by_name():
    net = room_model()
    batch = workloads.mp3d_like_batch(3, seed=7).to(DEV)
    nat = net.native()
    dead = [c.edge_type for c in nat.layers[-1].convs if not c.active]
    assert dead and all(e[2] == "objects" for e in dead)
    assert set(net.attention(batch)) == {c.edge_type for c in nat.layers[-1].convs if c.active}
    for e in dead:
        with pytest.raises(_lib.HydraMPError, match="inactive"):
            nat.attention(batch, 1, edge_types=[e])
        with pytest.raises(_lib.HydraMPError, match="inactive"):
            net.top_attended(batch, edge_type=e, k=2)
    # the library's own refusals, behind the Python checks
    h = nat.make_batch(batch)
    flat = nat.flat_params()
    lib = nat._lib
    buf = torch.zeros(1 << 16, device=DEV)
    slots = (C.c_void_p * _lib.MAX_EDGE_TYPES)()
    slots[nat.edge_types.index(dead[0])] = buf.data_ptr()
    rc = lib.hmp_net_attention(nat._handle, C.byref(h.c), flat.data_ptr(), 1, slots, 1, None, None, _lib.stream_ptr())
    assert rc == 1 and b"inactive" in lib.hmp_last_error() and b"layer 1" in lib.hmp_last_error()
    live = (C.c_void_p * _lib.MAX_EDGE_TYPES)()
    live[nat.edge_types.index(nat.attention_edge_types(1)[0])] = buf.data_ptr()
    for layer, k, what in ((2, 1, b"out of range"), (-1, 1, b"out of range"), (1, 0, b"k = "), (1, 9, b"k = ")):
        rc = lib.hmp_net_attention(nat._handle, C.byref(h.c), flat.data_ptr(), layer, live, k, None, None, _lib.stream_ptr())
        assert rc == 1 and what in lib.hmp_last_error(), (layer, k, lib.hmp_last_error())
    sage = HeterogeneousNetwork({"objects": 306, "rooms": 6}, output_dim=26, conv_block="GraphSAGE", hidden_dim=8, num_layers=2).to(DEV).eval()
    sage.predict_labels(batch)  # builds and binds the program
    sn = sage.native()
    rc = lib.hmp_net_attention(sn._handle, C.byref(sn.make_batch(batch).c), sn.flat_params().data_ptr(), 0, live, 1, None, None,
                               _lib.stream_ptr())
    assert rc == 1 and b"not a GAT layer" in lib.hmp_last_error()
    with pytest.raises(_lib.HydraMPError, match="no attention coefficients: conv_block GraphSAGE"):
        sage.attention(batch)


@pytest.mark.parametrize("block", BLOCKS)
def test_explain_rooms_is_top_attended_on_the_host(block):
    net = room_model(block)
    batch = workloads.mp3d_like_batch(3, seed=9, relative_pos=(block == "GAT_edge")).to(DEV)
    et = ("objects", "objects_to_rooms", "rooms")
    before = net.predict_labels(batch).clone()
    src, w = net.top_attended(batch, edge_type=et, k=3)
    hs, hw = net.explain_rooms(batch, k=3)
    n_rooms = int(batch["rooms"].x.size(0))
    assert not hs.is_cuda and not hw.is_cuda and tuple(hs.shape) == tuple(hw.shape) == (n_rooms, 3)
    assert torch.equal(hs, src.cpu()) and torch.equal(hw.view(torch.int32), w.cpu().view(torch.int32))
    # every named object is a neighbour of its room, weights descend, and padding is -1 / 0
    ei = batch[et].edge_index.cpu()
    for r in range(n_rooms):
        objs = set(ei[0][ei[1] == r].tolist())
        named = [int(v) for v in hs[r] if v >= 0]
        assert set(named) <= objs and len(named) == min(3, len(objs)), r
        assert bool((hw[r][:-1] >= hw[r][1:]).all()) and bool((hw[r][len(named):] == 0).all())
    # caller-owned buffers are written and a view returned; bad ones are refused
    sb, wb = torch.full((n_rooms + 2, 3), -7, dtype=torch.int64, device=DEV), torch.full((n_rooms + 2, 3), -7.0, device=DEV)
    vs, vw = net.native().top_attended(batch, 1, et, 3, out=(sb, wb))
    assert vs.data_ptr() == sb.data_ptr() and torch.equal(vs, src) and torch.equal(vw, w) and bool((sb[n_rooms:] == -7).all())
    for bad in ((sb[:n_rooms - 1], wb), (sb, wb.double()), (sb.cpu(), wb), (sb, wb[:, :2]), sb):
        with pytest.raises(_lib.HydraMPError, match="out"):
            net.native().top_attended(batch, 1, et, 3, out=bad)
    # calling attention changes nothing that predict_labels returns afterwards
    net.attention(batch, layer=0)
    assert torch.equal(net.predict_labels(batch), before)


@pytest.mark.parametrize("shape", SHAPES)
def test_attention_enqueues_the_forward_plus_one_launch(shape):
    _, net = pair_of(shape, "GAT", seed=13)
    batch = coll(shape, graphs_of(shape, "GAT", 3, seed=51)).to(DEV)
    view = net._view(batch) if shape.startswith("homog") else batch
    n_fwd = launches(net, lambda: net.native().forward(view, False))
    for layer in list(range(net.num_layers)) + (["pre_mp"] if "htree" in shape else []):
        n_att = launches(net, lambda: net.attention(batch, layer=layer))
        n_top = launches(net, lambda: net.top_attended(batch, k=3, layer=layer))
        print(shape, layer, "attention", n_att, "top", n_top, "forward", n_fwd)
        want = [v + (1 if k == KC_GAT_FWD else 0) for k, v in enumerate(n_fwd)]
        assert n_att == want and n_top == want
