"""Input gradients and gradient saliency through the executor, on every natively executed model class, against the
``oracle.models`` twin in float64 (tests/_saliency_reference.py: ``x.double().requires_grad_()``, sum of the selected logits or
log-probabilities, ``.backward()``).

Bound: ATOL = RTOL = 1e-5, test_gpu_models.py's bound for gradients.  For the ReLU (GraphSAGE) models the oracle also reports the
smallest |pre-activation| over all ReLU inputs of the run; the seeds below are chosen so that it is at least 1e-4 (checked on
the CPU: the oracle needs no device), far above the fp32 error of a pre-activation, so the two sides take the same ReLU branch
everywhere and a flipped branch can neither fail nor excuse the comparison.

Bit-level checks (same kernels on the same bytes): ``target=None`` against ``target=predict_labels``, the autograd idiom
``x.requires_grad_(); model(data)[i, c].backward()`` against ``input_gradients`` of that row and class, stream descriptors against
host batches, ``saliency`` against the unit score entry, ``top_salient`` / ``explain_rooms`` against ``top_from_scores`` of the exact
per-room scores, and a training step after the calls against a twin net that never made them."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hydra_gnn_amd import _lib, workloads  # noqa: E402
from hydra_gnn_amd.data import HeteroData, collate, collate_homogeneous  # noqa: E402
from hydra_gnn_amd.models import (HeterogeneousNetwork, HeterogeneousNeuralTreeNetwork, HomogeneousNetwork,  # noqa: E402
                                  HomogeneousNeuralTreeNetwork)
from hydra_gnn_amd.store import GraphStore  # noqa: E402
from oracle import models as omodels  # noqa: E402
from _saliency_reference import oracle_input_gradients, scores_reference, top_from_scores  # noqa: E402

ATOL, RTOL = 1e-5, 1e-5
RELU_MARGIN = 1e-4
DEV = "cuda:0"
HT_DIMS = {"object": 306, "room": 6, "object-room": 6, "room-room": 6, "object_virtual": 306, "room_virtual": 6}
GAT = dict(GAT_hidden_dims=[8], GAT_heads=[2, 2], GAT_concats=[True, False])
O2R = ("objects", "objects_to_rooms", "rooms")


def ragged_batch():
    """the two-graph case of test_gpu_models.test_empty_and_ragged_edge_types: an empty edge type, orphan objects, a one-room graph"""
    rng = np.random.default_rng(3)
    gs = []
    for n_rooms in (2, 1):
        g = HeteroData()
        g["objects"].x = torch.from_numpy(rng.normal(size=(5, 306)).astype(np.float32))
        g["rooms"].x = torch.from_numpy(rng.normal(size=(n_rooms, 6)).astype(np.float32))
        g["rooms"].y = torch.tensor([3, 25][:n_rooms])
        g["objects", "objects_to_objects", "objects"].edge_index = torch.tensor([[0, 1, 1], [1, 0, 0]])  # duplicate edge
        g["rooms", "rooms_to_rooms", "rooms"].edge_index = torch.empty((2, 0), dtype=torch.int64)
        last = n_rooms - 1
        g["rooms", "rooms_to_objects", "objects"].edge_index = torch.tensor([[0, 0, last], [0, 1, 4]])  # objects 2, 3 orphaned
        g["objects", "objects_to_rooms", "rooms"].edge_index = torch.tensor([[0, 1, 4, 1], [0, 0, last, 0]])  # object 1 twice
        gs.append(g)
    return gs


# name -> (class, oracle class, constructor arguments, graphs(seed), collate, model seed, graph seed, head, has ReLU)
def _mp3d(n, **kw):
    return lambda seed: [workloads.mp3d_like_graph(g, **kw) for g in [np.random.Generator(np.random.PCG64(seed))] for _ in range(n)]


def _relpos(graphs):
    from hydra_gnn_amd.data import compute_relative_pos

    for g in graphs:
        compute_relative_pos(g)
    return graphs


def _htree(n):
    def make(seed):
        npz = np.load(workloads.HTREE_FIXTURE)
        rng = np.random.Generator(np.random.PCG64(seed))
        return [workloads.htree_graph(npz, i % int(npz["n_graphs"]), rng) for i in range(n)]
    return make


def _stanford(n):
    def make(seed):
        rng = np.random.Generator(np.random.PCG64(seed))
        return [workloads.stanford_like_graph(rng, n_nodes=(2 if i == 0 else None)) for i in range(n)]
    return make


def _homog_htree(n):
    def make(seed):
        from hydra_gnn_amd.data import heterogeneous_htree_to_homogeneous

        out = []
        for g in _htree(n)(seed):
            d = heterogeneous_htree_to_homogeneous(g)
            del d.__dict__["edge_type"]  # per-edge attribute of edge_index only (would be concatenated with the wrong length)
            d.x = d.x[:, :6].contiguous()
            out.append(d)
        return out
    return make


HET = dict(input_dim_dict={"objects": 306, "rooms": 6})
CASES = {
    "sage32x2": (HeterogeneousNetwork, omodels.HeterogeneousNetwork,
                 dict(HET, output_dim=26, conv_block="GraphSAGE", hidden_dim=32, num_layers=2, dropout=0.0), _mp3d(6), collate, 0, 11, None, True),
    "sage32x3": (HeterogeneousNetwork, omodels.HeterogeneousNetwork,
                 dict(HET, output_dim=26, conv_block="GraphSAGE", hidden_dim=32, num_layers=3, dropout=0.0), _mp3d(6), collate, 160, 12, None, True),
    "ragged": (HeterogeneousNetwork, omodels.HeterogeneousNetwork,
               dict(HET, output_dim=26, conv_block="GraphSAGE", hidden_dim=16, num_layers=3, dropout=0.0), lambda seed: ragged_batch(), collate,
               2, 0, None, True),
    "gat": (HeterogeneousNetwork, omodels.HeterogeneousNetwork, dict(HET, output_dim=26, conv_block="GAT", dropout=0.0, **GAT), _mp3d(6),
            collate, 3, 13, None, False),
    "gat_edge": (HeterogeneousNetwork, omodels.HeterogeneousNetwork,
                 dict(input_dim_dict={"objects": 303, "rooms": 3}, output_dim=26, conv_block="GAT_edge", dropout=0.0, **GAT),
                 lambda seed: _relpos(_mp3d(6)(seed)), collate, 4, 14, None, False),
    "two_head_rooms": (HeterogeneousNetwork, omodels.HeterogeneousNetwork,
                       dict(HET, output_dim_dict={"rooms": 26, "objects": 35}, conv_block="GraphSAGE", hidden_dim=32, num_layers=2, dropout=0.0),
                       _mp3d(5), collate, 101, 15, 0, True),
    "two_head_objects": (HeterogeneousNetwork, omodels.HeterogeneousNetwork,
                         dict(HET, output_dim_dict={"rooms": 26, "objects": 35}, conv_block="GraphSAGE", hidden_dim=32, num_layers=2, dropout=0.0),
                         _mp3d(5), collate, 101, 15, 1, True),
    "htree_gat": (HeterogeneousNeuralTreeNetwork, omodels.HeterogeneousNeuralTreeNetwork,
                  dict(input_dim_dict=HT_DIMS, output_dim=26, conv_block="GAT", GAT_hidden_dims=[16], GAT_heads=[2, 2], GAT_concats=[True, False],
                       disable_initialization=False, dropout=0.0), _htree(5), collate, 6, 33, None, False),
    "htree_sage": (HeterogeneousNeuralTreeNetwork, omodels.HeterogeneousNeuralTreeNetwork,
                   dict(input_dim_dict=HT_DIMS, output_dim=26, conv_block="GraphSAGE", hidden_dim=8, num_layers=2, disable_initialization=True,
                        dropout=0.0), _htree(2), collate, 7, 34, None, True),
    "homog_sage": (HomogeneousNetwork, omodels.HomogeneousNetwork,
                   dict(input_dim=6, output_dim=15, conv_block="GraphSAGE", hidden_dim=32, num_layers=2, dropout=0.0), _stanford(5),
                   collate_homogeneous, 8, 35, None, True),
    "homog_htree_gat": (HomogeneousNeuralTreeNetwork, omodels.HomogeneousNeuralTreeNetwork,
                        dict(input_dim=6, output_dim=26, conv_block="GAT", GAT_hidden_dims=[16, 16], GAT_heads=[2, 2, 2],
                             GAT_concats=[True, True, False], disable_initialization=False, dropout=0.0), _homog_htree(4), collate_homogeneous,
                        9, 41, None, False),
}
MODEL_CASES = tuple(CASES)


def host_case(name, dropout=None):
    """(oracle, engine model on the host, graphs, collate, head, relu) of a case: needs no device"""
    cls, ocls, kw, graphs, coll, mseed, gseed, head, relu = CASES[name]
    kw = dict(kw) if dropout is None else dict(kw, dropout=dropout)
    torch.manual_seed(mseed)
    ora = ocls(**kw)
    with torch.no_grad():  # the oracle's GATConv bias starts at zero
        for pname, p in ora.named_parameters():
            if pname.endswith("bias") and kw["conv_block"][:3] == "GAT":
                p.uniform_(-0.1, 0.1)
    net = cls(**kw)
    net.load_state_dict(ora.state_dict(), strict=True)
    return ora, net, graphs(gseed), coll, head, relu


def homog(batch):
    return not hasattr(batch, "node_types")


def native_args(batch, head, target=None, rows=None):
    """the engine's (target, rows) for the oracle's: homogeneous models take one entry per NODE, the oracle's rows are the
    room_mask rows in order"""
    if not homog(batch):
        return (target.to(DEV) if target is not None else None, rows.to(DEV) if rows is not None else None)
    idx, n = torch.nonzero(batch.room_mask).flatten(), int(batch.x.size(0))
    t = r = None
    if target is not None:
        t = torch.zeros(n, dtype=torch.int64)
        t[idx] = target
        t = t.to(DEV)
    if rows is not None:
        r = torch.zeros(n, dtype=torch.bool)
        r[idx] = rows
        r = r.to(DEV)
    return t, r


def as_dict(res):
    return {None: res} if isinstance(res, torch.Tensor) else res


def check_close(got, ref, tag):
    got, ref = as_dict(got), dict(ref)
    assert set(got) <= set(ref), tag
    for t, g in got.items():
        r = ref[t]
        err = float((g.cpu().double() - r).abs().max()) if r.numel() else 0.0
        print(f"{tag} [{t}]: max |gx - oracle| = {err:.3e} (max |oracle| = {float(r.abs().max()) if r.numel() else 0.0:.3e})")
        assert tuple(g.shape) == tuple(r.shape) and g.dtype == torch.float32 and g.is_cuda, f"{tag} [{t}]"
        torch.testing.assert_close(g.cpu().double(), r, atol=ATOL, rtol=RTOL, msg=lambda m: f"{tag} [{t}]: {m}")


def bits_equal(a, b):
    a, b = as_dict(a), as_dict(b)
    return set(a) == set(b) and all(torch.equal(a[t].contiguous().view(torch.int32), b[t].contiguous().view(torch.int32)) for t in a)


@pytest.mark.parametrize("name", MODEL_CASES)
def test_input_gradients_equal_the_oracle(name):
    ora, net, graphs, coll, head, relu = host_case(name)
    net = net.to(DEV).eval()
    host = coll(graphs)
    batch = coll(graphs).to(DEV)
    kw = {} if head is None else {"head": head}
    grads, margin, logits = oracle_input_gradients(ora, coll(graphs), head=head)
    if relu:
        assert margin >= RELU_MARGIN, f"{name}: smallest |ReLU input| of the oracle is {margin:.3e}: pick another seed"
    n_out, n_cls = logits.shape
    g_all = net.input_gradients(batch, **kw)
    check_close(g_all, grads, f"{name} logit, predicted class, all rows")
    # target=None is target=predict_labels: the same bits
    labels = net.predict_labels(batch)
    labels = labels[head] if isinstance(labels, tuple) else labels
    assert bits_equal(g_all, net.input_gradients(batch, target=labels.clamp(min=0), **kw)), name
    rng = np.random.default_rng(len(name))
    target = torch.from_numpy(rng.integers(0, n_cls, n_out))
    rows = torch.from_numpy(rng.integers(0, 2, n_out).astype(bool))
    rows[0] = True
    for wrt, tg, rw in (("logprob", None, None), ("logit", target, None), ("logprob", target, rows), ("logit", None, rows)):
        ref, _, _ = oracle_input_gradients(ora, coll(graphs), target=tg, rows=rw, wrt=wrt, head=head)
        t, r = native_args(host, head, tg, rw)  # (rows None: all output rows; a homogeneous model's default is its room_mask)
        got = net.input_gradients(batch, target=t, rows=r, wrt=wrt, **kw)
        check_close(got, ref, f"{name} {wrt} target={'given' if tg is not None else 'predicted'} rows={'mask' if rw is not None else 'all'}")
    # exact per-row passes in ordinal mode add up to the pass over all rows
    nat = net.native()
    view = net._attention_input(batch)
    h = nat.make_batch(view)
    if not homog(host):  # (the rooms of a homogeneous batch are not its graphs' leading rows: it selects them by mask)
        passes = nat.max_graph_rows(h, nat.head_type(head or 0))
        total = None
        for p in range(passes):
            part = {t: g.clone() for t, g in nat.input_gradients(h, ordinal=p, head=head or 0).items()}
            total = part if total is None else {t: total[t] + part[t] for t in total}
        for t, g in as_dict(g_all).items():
            torch.testing.assert_close(total[t], g, atol=ATOL, rtol=RTOL, msg=lambda m: f"{name} ordinal sum [{t}]: {m}")
        assert passes <= n_out


@pytest.mark.parametrize("name", ["sage32x2", "gat", "two_head_objects", "htree_gat", "homog_sage", "homog_htree_gat"])
def test_autograd_gives_the_bits_of_input_gradients(name):
    ora, net, graphs, coll, head, relu = host_case(name)
    net = net.to(DEV).eval()
    host = coll(graphs)
    batch = coll(graphs).to(DEV)
    hom = homog(host)
    xs = {None: batch.x} if hom else {t: batch[t].x for t in batch.node_types if "x" in batch[t]}
    for x in xs.values():
        x.requires_grad_()
    out = net(batch)
    out = out[head] if head is not None else out
    i, c = out.size(0) - 1, 3
    out[i, c].backward()
    rows = torch.zeros(out.size(0), dtype=torch.bool)
    rows[i] = True
    target = torch.full((out.size(0),), c, dtype=torch.int64)
    t, r = native_args(host, head, target, rows)
    want = as_dict(net.input_gradients(batch, target=t, rows=r, **({} if head is None else {"head": head})))
    seen = 0
    for key, x in xs.items():
        if key not in want:
            assert x.grad is None or not bool(x.grad.any()), key
            continue
        assert x.grad is not None and x.grad.shape == x.shape, f"{name} [{key}]: x.grad is missing"
        assert torch.equal(x.grad.view(torch.int32), want[key].contiguous().view(torch.int32)), f"{name} [{key}]: x.grad differs"
        seen += int(bool(x.grad.any()))
    assert seen > 0
    # without requires_grad nothing about the call changes
    plain = coll(graphs).to(DEV)
    with torch.no_grad():
        again = net(plain)
    again = again[head] if head is not None else again
    assert torch.equal(again, out.detach())


def test_training_mode_autograd_replays_the_dropout_masks():
    """a training-mode GraphSAGE forward with dropout 0.25: x.grad against the oracle replaying the engine's keep-masks"""
    from test_gpu_models import hetero_replay

    ora, net, graphs, coll, head, relu = host_case("sage32x3", dropout=0.25)
    # The dropout seed is part of this run's inputs: under the masks of the seed the model drew, the smallest |ReLU input| of the
    # oracle is 9.5e-5, below the margin; under those of seed + 2 it is 4.8e-4 (found on the CPU by replaying the masks of
    # tests/_dropout_reference.py in the oracle: seed + 1 gives 5.1e-5).
    net._seed += 2
    net = net.to(DEV).train()
    batch = coll(graphs).to(DEV)
    for t in ("objects", "rooms"):
        batch[t].x.requires_grad_()
    out = net(batch)  # rng_step becomes 1
    n_out, n_cls = out.shape
    rng = np.random.default_rng(7)
    target = torch.from_numpy(rng.integers(0, n_cls, n_out))
    out[torch.arange(n_out), target.to(DEV)].sum().backward()
    ora.dropout_fn = hetero_replay(net)
    ref, margin, logits = oracle_input_gradients(ora, coll(graphs), target=target, train=True)
    assert margin >= RELU_MARGIN, f"smallest |ReLU input| of the oracle is {margin:.3e}: pick another seed"
    torch.testing.assert_close(out.detach().cpu().double(), logits, atol=ATOL, rtol=RTOL)
    check_close({t: batch[t].x.grad for t in ("objects", "rooms")}, ref, "training-mode sage32x3")


def store_graphs(name):
    """graphs a GraphStore takes for the case (labels of the readout rows present)"""
    ora, net, graphs, coll, head, relu = host_case(name)
    return net.to(DEV).eval(), graphs, coll


@pytest.mark.parametrize("name,label_type", [("sage32x2", "rooms"), ("gat_edge", "rooms"), ("htree_gat", "room_virtual"), ("homog_sage", "node")])
def test_stream_descriptors_give_the_bits_of_host_batches(name, label_type):
    net, graphs, coll = store_graphs(name)
    store = GraphStore(graphs, DEV)
    stream = store.stream(net, 4, label_type=label_type)
    for ids in ([0, 1, 2], [4], [3, 3, 1, 0]):
        host = coll([graphs[i] for i in ids]).to(DEV)
        for wrt in ("logit", "logprob"):
            want = net.input_gradients(host, wrt=wrt)
            got = net.input_gradients(stream.next(ids), wrt=wrt)
            assert bits_equal(want, got), (name, ids, wrt)
        ws, gs = net.saliency(host), net.saliency(stream.next(ids))
        ws, gs = ({None: ws}, {None: gs}) if isinstance(ws, tuple) else (ws, gs)
        for t in ws:
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(ws[t], gs[t])), (name, ids, t)
    if name == "sage32x2":
        want = net.explain_rooms(coll([graphs[i] for i in (0, 2, 5)]).to(DEV), k=3, by="gradient")
        want = (want[0].clone(), want[1].clone())
        got = net.explain_rooms(stream.next([0, 2, 5]), k=3, by="gradient")
        assert torch.equal(want[0], got[0]) and torch.equal(want[1].view(torch.int32), got[1].view(torch.int32))


@pytest.mark.parametrize("name", ["sage32x3", "gat_edge", "homog_sage"])
def test_saliency_is_the_unit_entry_on_input_gradients(name):
    ora, net, graphs, coll, head, relu = host_case(name)
    net = net.to(DEV).eval()
    batch = coll(graphs).to(DEV)
    lib = _lib.require_device()
    groups = ((0, 3), (3, 6), (6, None), (2, 5))
    gx = as_dict(net.input_gradients(batch, wrt="logprob"))
    sal = net.saliency(batch, groups=groups, wrt="logprob")
    sal = {None: sal} if isinstance(sal, tuple) else sal
    assert set(sal) == set(gx)
    for t, (gxi, gnorm, grp) in sal.items():
        x = batch.x if t is None else batch[t].x
        n, F = x.shape
        g = gx[t].contiguous()
        lo = (C.c_int32 * 4)(*[a for a, _ in groups])
        hi = (C.c_int32 * 4)(*[F if b is None else min(b, F) for _, b in groups])
        o1, o2, o3 = torch.empty(n, device=DEV), torch.empty(n, device=DEV), torch.empty(n, 4, device=DEV)
        _lib.check(lib.hmp_saliency_scores(g.data_ptr(), F, x.data_ptr(), x.stride(0), n, F, 4, lo, hi, o1.data_ptr(), o2.data_ptr(),
                                           o3.data_ptr(), _lib.stream_ptr()))
        assert tuple(gxi.shape) == tuple(gnorm.shape) == (n,) and tuple(grp.shape) == (n, 4), (name, t)
        for a, b in ((gxi, o1), (gnorm, o2), (grp, o3)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, t)
        ref = scores_reference(g.cpu().numpy(), x.detach().cpu().numpy(), F, groups)
        assert (np.abs(gxi.cpu().numpy() - ref[0]) <= ATOL * ref[3]).all(), (name, t)
    with pytest.raises(_lib.HydraMPError, match="column groups"):
        net.saliency(batch, groups=((0, 1),) * 5)


def per_room_reference(net, batch, et, k, **kw):
    """top_from_scores of every room's own exact scores: one masked input-gradient pass per room"""
    nat = net.native()
    h = nat.make_batch(batch)
    si = nat.node_types.index(et[0])
    n_dst = h.n_nodes[nat.node_types.index(et[2])]
    ei = batch[et].edge_index.cpu().numpy()
    src = np.full((n_dst, k), -1, dtype=np.int64)
    sco = np.zeros((n_dst, k), dtype=np.float32)
    for r in range(n_dst):
        rows = torch.zeros(n_dst, dtype=torch.bool, device=DEV)
        rows[r] = True
        gxi = nat.saliency(h, groups=(), rows=rows, **kw)[et[0]][0].cpu().numpy()
        sel = np.zeros(n_dst, dtype=bool)
        sel[r] = True
        s, w = top_from_scores(gxi, ei, h.n_nodes[si], n_dst, k, sel)
        src[r], sco[r] = s[r], w[r]
    return src, sco


@pytest.mark.parametrize("name", ["sage32x2", "ragged", "gat"])
def test_explain_rooms_ranks_the_exact_per_room_scores(name):
    ora, net, graphs, coll, head, relu = host_case(name)
    net = net.to(DEV).eval()
    batch = coll(graphs).to(DEV)
    before = net.predict_labels(batch).clone()
    n_rooms = int(batch["rooms"].x.size(0))
    for k in (1, 3):
        want_src, want_sco = per_room_reference(net, batch, O2R, k)
        hs, hw = net.explain_rooms(batch, k=k, by="gradient")
        assert not hs.is_cuda and not hw.is_cuda and tuple(hs.shape) == tuple(hw.shape) == (n_rooms, k)
        assert np.array_equal(hs.numpy(), want_src), f"{name} k={k}: objects differ"
        assert np.array_equal(hw.numpy().view(np.uint32), want_sco.view(np.uint32)), f"{name} k={k}: scores differ"
        ds, dw = net.native().top_salient(batch, O2R, k, passes=net.native().max_graph_rows(batch, "rooms"))
        assert ds.is_cuda and np.array_equal(ds.cpu().numpy(), want_src) and np.array_equal(dw.cpu().numpy().view(np.uint32), want_sco.view(np.uint32))
    # one gradient for all rooms: top_from_scores of saliency's gxi, for every live conv with input features behind it
    top = net.top_salient(batch, k=3)
    sal = net.saliency(batch)
    assert O2R in top and all(e in net.native().salient_edge_types() for e in top)
    for et, (src, sco) in top.items():
        n_src, n_dst = batch[et[0]].x.size(0), batch[et[2]].x.size(0)
        s, w = top_from_scores(sal[et[0]][0].cpu().numpy(), batch[et].edge_index.cpu().numpy(), n_src, n_dst, 3)
        assert np.array_equal(src.cpu().numpy(), s) and np.array_equal(sco.cpu().numpy().view(np.uint32), w.view(np.uint32)), (name, et)
    one = net.top_salient(batch, edge_type=O2R, k=3)
    assert torch.equal(one[0], top[O2R][0]) and torch.equal(one[1], top[O2R][1])
    if name == "gat":  # GAT models keep returning the attention form by default
        att = net.explain_rooms(batch, k=3)
        ts, tw = net.top_attended(batch, edge_type=O2R, k=3)
        assert torch.equal(att[0], ts.cpu()) and torch.equal(att[1], tw.cpu()) and bool((att[1] >= 0).all())
    else:
        with pytest.raises(_lib.HydraMPError, match="no attention coefficients: conv_block GraphSAGE"):
            net.explain_rooms(batch, k=3, by="attention")
    assert torch.equal(net.predict_labels(batch), before)


def test_htree_explain_rooms_ranks_the_leaves_of_the_pool():
    ora, net, graphs, coll, head, relu = host_case("htree_sage")
    net = net.to(DEV).eval()
    batch = coll(graphs).to(DEV)
    et = ("room", "r_to_rv", "room_virtual")
    want_src, want_sco = per_room_reference(net, batch, et, 2)
    hs, hw = net.explain_rooms(batch, k=2)
    assert np.array_equal(hs.numpy(), want_src) and np.array_equal(hw.numpy().view(np.uint32), want_sco.view(np.uint32))


@pytest.mark.parametrize("name", ["homog_sage", "homog_htree_gat"])
def test_homogeneous_explain_rooms_ranks_each_rooms_neighbours(name):
    ora, net, graphs, coll, head, relu = host_case(name)
    net = net.to(DEV).eval()
    batch = coll(graphs).to(DEV)
    nat = net.native()
    n = int(batch.x.size(0))
    rooms = torch.nonzero(batch.room_mask).flatten().tolist()
    ei = (batch.pool_edge_index if name == "homog_htree_gat" else batch.edge_index).cpu().numpy()
    hs, hw = net.explain_rooms(batch, k=2)
    assert not hs.is_cuda and tuple(hs.shape) == tuple(hw.shape) == (len(rooms), 2)
    for i, r in enumerate(rooms):
        rows = torch.zeros(n, dtype=torch.bool, device=DEV)
        rows[r] = True
        gxi = nat.saliency(net._view(batch), groups=(), rows=rows)["node"][0].cpu().numpy()
        sel = np.zeros(n, dtype=bool)
        sel[r] = True
        s, w = top_from_scores(gxi, ei, n, n, 2, sel)
        assert np.array_equal(hs[i].numpy(), s[r]) and np.array_equal(hw[i].numpy().view(np.uint32), w[r].view(np.uint32)), (name, r)
    assert bool((hs[:, 0] >= 0).any()), "no room has a source to rank"


def step_state(net, step):
    torch.cuda.synchronize()
    return [step.loss()] + [p.detach().clone() for p in net.parameters()] + [step.m.clone(), step.v.clone()]


@pytest.mark.parametrize("name", ["sage32x3", "gat"])
def test_a_training_step_after_the_calls_is_the_twins(name):
    """loss, parameters and Adam moments of a step after saliency calls equal those of a twin net that never made them"""
    states = []
    for explain in (False, True):
        ora, net, graphs, coll, head, relu = host_case(name, dropout=0.25 if name != "gat" else None)
        net = net.to(DEV)
        batch = coll(graphs).to(DEV)
        y = batch["rooms"].y
        step = net.train_step(lr=0.002, weight_decay=0.001, ignored_label=25, seed=3)
        step(batch, y)
        if explain:
            net.eval()
            net.input_gradients(batch, wrt="logprob")
            net.saliency(batch)
            net.top_salient(batch, k=2)
            net.explain_rooms(batch, k=2, by="gradient")
            net.train()
        step(batch, y)
        states.append(step_state(net, step))
    assert states[0][0] == states[1][0], "loss differs"
    for a, b in zip(states[0][1:], states[1][1:]):
        assert torch.equal(a, b)


def test_refusals_of_the_entry():
    ora, net, graphs, coll, head, relu = host_case("sage32x2")
    net = net.to(DEV).eval()
    batch = coll(graphs).to(DEV)
    net.predict_labels(batch)  # builds and binds the program
    nat = net.native()
    h, flat, lib = nat.make_batch(batch), nat.flat_params(), nat._lib
    slots = (C.c_void_p * _lib.MAX_NODE_TYPES)()
    call = lambda head, mode, wrt, mask=None, ptr=None: lib.hmp_net_input_gradient(  # noqa: E731
        nat._handle, C.byref(h.c), flat.data_ptr(), head, None, mode, mask, 0, ptr, 0, wrt, slots, _lib.stream_ptr())
    for args, what in (((1, 0, 0), b"head 1"), ((0, 3, 0), b"selection mode"), ((0, 1, 0), b"mask"), ((0, 2, 0), b"ordinal"), ((0, 0, 2), b"wrt")):
        assert call(*args) == 1 and what in lib.hmp_last_error(), (args, lib.hmp_last_error())
    nat.set_compute("bf16")
    assert call(0, 0, 0) == 1 and b"bf16" in lib.hmp_last_error()
    with pytest.raises(_lib.HydraMPError, match="bf16"):
        net.input_gradients(batch)
    nat.set_compute("fp32")
    with pytest.raises(_lib.HydraMPError, match="overlap"):
        nat.input_gradients(batch, rows=torch.ones(h.c.n_out, dtype=torch.bool, device=DEV), ordinal=0)
    with pytest.raises(_lib.HydraMPError, match="another model"):
        other = host_case("sage32x2")[1].to(DEV).eval()
        stream = GraphStore(graphs, DEV).stream(other, 4, label_type="rooms")
        net.input_gradients(stream.next([0, 1]))


# ---- evaluate.saliency and the training job's saliency() ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,label_type", [("sage32x2", "rooms"), ("homog_sage", "node")])
def test_evaluate_saliency_over_a_stream_reads_the_device_once(name, label_type, monkeypatch):
    """6 (5) graphs in batches of 4: per-graph arrays equal the per-batch calls sliced by the store's node counts"""
    from hydra_gnn_amd import evaluate, jobs
    from test_gpu_predict_models import ReadCounter

    net, graphs, coll = store_graphs(name)
    store = GraphStore(graphs, DEV)
    stream = store.stream(net, 4, label_type=label_type)
    chunks = jobs.id_chunks(len(graphs), 4)
    evaluate.saliency(net, (stream, chunks))  # warm
    torch.cuda.synchronize()
    with monkeypatch.context() as m:
        counter = ReadCounter(m)
        got = evaluate.saliency(net, (stream, chunks), wrt="logprob")
    assert counter.n == 1, counter.by
    assert len(got) == len(graphs)
    g = 0
    for ids in chunks:
        sal = net.saliency(coll([graphs[i] for i in ids]).to(DEV), wrt="logprob")
        sal = {None: sal} if isinstance(sal, tuple) else sal
        off = {t: 0 for t in sal}
        for i in ids:
            piece = {None: got[g]} if isinstance(got[g], tuple) else got[g]
            assert set(piece) == set(sal)
            for t, trip in sal.items():
                n = int(graphs[i].x.size(0) if t is None else graphs[i][t].x.size(0))
                for a, b in zip(piece[t], trip):
                    assert a.dtype == np.float32 and np.array_equal(a.view(np.uint32), b[off[t]:off[t] + n].cpu().numpy().view(np.uint32)), (name, i, t)
                off[t] += n
            g += 1
    per_batch = evaluate.saliency(net, [coll([graphs[i] for i in ids]).to(DEV) for ids in chunks])
    assert len(per_batch) == len(chunks)


def test_room_job_saliency():
    from hydra_gnn_amd import jobs
    from test_gpu_predict_models import GraphDataset, opt

    rng = np.random.default_rng(31)
    gs = [workloads.mp3d_like_graph(rng) for _ in range(14)]
    feats = {"objects": 306, "rooms": 6}
    dd = {"train": GraphDataset("heterogeneous", gs[:4], feats, 26), "val": GraphDataset("heterogeneous", gs[4:6], feats, 26),
          "test": GraphDataset("heterogeneous", gs[6:], feats, 26)}
    torch.manual_seed(3)
    job = jobs.BaseTrainingJob(dd, dict(conv_block="GraphSAGE", hidden_dim=32, num_layers=3))
    opt(job)
    job._net.to(DEV)
    sal = job.saliency("test")
    assert len(sal) == 8
    for g, piece in zip(gs[6:], sal):
        assert set(piece) == {"objects", "rooms"}
        for t, (gxi, gnorm, grp) in piece.items():
            n = int(g[t].x.size(0))
            assert gxi.shape == gnorm.shape == (n,) and grp.shape == (n, 3) and bool((gnorm >= 0).all())
            np.testing.assert_allclose(grp.sum(axis=1), gxi, atol=1e-5 * max(1.0, float(np.abs(grp).sum(axis=1).max())))
    gin = jobs.BaseTrainingJob({k: GraphDataset("homogeneous", [workloads.stanford_like_graph(rng) for _ in range(3)], 6, 15) for k in dd},
                               dict(conv_block="GIN", hidden_dim=8, num_layers=2))
    with pytest.raises(_lib.HydraMPError, match="GIN models run op by op"):
        gin.saliency("test")
