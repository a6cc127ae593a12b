"""The gradient un-pack (grad_reduce_kernel: split-K slab sums, de-stacking, Adam in the same launch for SAGE nets) on every path
of its workgroup records, against the float64 oracle and ``torch.optim.Adam`` the way tests/test_gpu_fusion.py compares: the flat
gradient after one backward at ATOL / RTOL, the parameters and Adam's moments after two steps by that file's step rule (no element
further than steps * lr * 2.1 from the oracle's, under 1 % of a tensor further than 2e-5: Adam divides by |g|, so where |g| ~ eps
a rounding of g moves the update by a fraction of lr).

Slab counts.  The small-batch weight gradients come from gemm_tn_direct_launch (csrc/gemm_direct.hip), whose rule for a problem
over K nodes with T output tiles of 32 x 32 is: ks = ceil(K / 384); doubled while 2 ks <= 16, ceil(K / 2 ks) >= 32 and T ks < 256;
then ks = ceil(K / kchunk) with kchunk = ceil(K / ks) rounded up to even.  The 2-layer hidden-64 net has T = 60 (objects) and 6
(rooms) in layer 0 and T = 9 in layer 1; K is the node count of the source type.  ``tn_slabs`` restates the rule and
``test_batches_reach_the_slab_counts`` shows what the four batches below reach: 1, 2, 4, 5, 8, 10 and 16 slabs -- one batch of
the un-pack's first 16, a partial batch, and terms of different depth in one launch.  More than 16 slabs come from the linear
heads, whose slab count is the head kernel's workgroup count ceil(rows / 32).
"""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from hydra_gnn_amd import workloads  # noqa: E402
from hydra_gnn_amd.models import HeterogeneousNetwork, HomogeneousNetwork  # noqa: E402
from oracle import models as omodels  # noqa: E402

ATOL, RTOL = 1e-5, 1e-5  # tests/test_gpu_fusion.py
DEV = "cuda:0"
LR, WD = 0.002, 0.001
STEPS = 2

SAGE2 = dict(input_dim_dict={"objects": 306, "rooms": 6}, output_dim=26, conv_block="GraphSAGE", hidden_dim=64, num_layers=2,
             dropout=0.0)


def cdiv(a, b):
    return -(-a // b)


def tn_slabs(K, tiles, max_slabs=16):
    """gemm_tn_direct_launch's slab count (module docstring)"""
    ks = max(cdiv(K, 384), 1)
    while ks * 2 <= max_slabs and cdiv(K, ks * 2) >= 32 and tiles * ks < 256:
        ks *= 2
    kchunk = max(cdiv(cdiv(K, ks), 2) * 2, 2)
    return cdiv(K, kchunk)


def to64(batch):
    b64 = batch.to("cpu")
    for t in b64.node_types:
        b64[t].x = b64[t].x.double()
    for et in b64.edge_types:
        if "edge_attr" in b64[et]:
            b64[et].edge_attr = b64[et].edge_attr.double()
    return b64


def oracle_steps(ora, batch, weight=None):
    """float64 oracle + torch.optim.Adam for STEPS steps: the mean-loss gradients of step 1, then parameters and moments"""
    o64 = copy.deepcopy(ora).double()
    o64.eval()
    opt = torch.optim.Adam(o64.parameters(), lr=LR, weight_decay=WD)
    b64 = to64(batch)
    y = batch["rooms"].y
    w64 = None if weight is None else torch.as_tensor(weight, dtype=torch.float64)
    grads = None
    for s in range(STEPS):
        opt.zero_grad()
        pred = o64(b64)
        if w64 is None:
            loss = o64.loss(pred, y, y != 25)
        else:
            loss = torch.nn.functional.cross_entropy(pred[y != 25], y[y != 25], weight=w64)
        loss.backward()
        if s == 0:
            grads = {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in o64.named_parameters()}
        opt.step()
    names = dict(o64.named_parameters())
    state = {n: opt.state[p] for n, p in names.items() if p in opt.state}
    return {"grads": grads, "p": {n: p.detach().clone() for n, p in names.items()},
            "m": {n: s["exp_avg"].clone() for n, s in state.items()}, "v": {n: s["exp_avg_sq"].clone() for n, s in state.items()}}


def pair(kw, seed=0, bias_noise=False):
    torch.manual_seed(seed)
    ora = omodels.HeterogeneousNetwork(**kw)
    if bias_noise:  # GATConv's bias starts at zero
        with torch.no_grad():
            for n, p in ora.named_parameters():
                if n.endswith(".bias"):
                    p.uniform_(-0.1, 0.1)
    return ora


def engine_of(ora, kw):
    net = HeterogeneousNetwork(**kw)
    net.load_state_dict(ora.state_dict(), strict=True)
    return net.to(DEV)


def step_rule(got, ref, what):
    """tests/test_gpu_fusion.py::test_fused_step_equals_two_phase_step's rule"""
    d = (got.detach().cpu().double() - ref).abs()
    assert float(d.max()) <= STEPS * LR * 2.1, what
    assert float((d > 2e-5).double().mean()) < 0.01, what


def check(ora, kw, batch, ref, weight=None, **step_kw):
    """one backward: every gradient against the oracle; STEPS training steps: p, m, v against the oracle's Adam"""
    net = engine_of(ora, kw)
    net.eval()
    gb = batch.to(DEV)
    y = gb["rooms"].y
    net.loss(net(gb), y, y != 25, **({} if weight is None else {"weight": weight})).backward()
    for name, p in net.named_parameters():
        g = ref["grads"][name]
        if g is None:
            assert p.grad is None, name
            continue
        torch.testing.assert_close(p.grad.cpu().double(), g, atol=ATOL, rtol=RTOL, msg=lambda m: f"{name}: {m}")
    net = engine_of(ora, kw)
    net.eval()
    step = net.train_step(lr=LR, weight_decay=WD, ignored_label=25, use_graph=False, training=False, class_weight=weight, **step_kw)
    for _ in range(STEPS):
        step(gb, y)
    torch.cuda.synchronize()
    assert net.native().read_state() == (STEPS, 0)
    off = net.native().param_offsets
    for name, p in net.named_parameters():
        step_rule(p, ref["p"][name], f"p {name}")
        if name in ref["m"]:
            o = off[id(p)]
            step_rule(step.m[o: o + p.numel()].view(p.shape), ref["m"][name], f"m {name}")
            step_rule(step.v[o: o + p.numel()].view(p.shape), ref["v"][name], f"v {name}")
    return net, step


@functools.lru_cache(maxsize=None)
def sage_case(n_graphs):
    ora = pair(SAGE2)
    batch = workloads.config2_batch(n_graphs)
    return ora, batch, oracle_steps(ora, batch)


BATCHES = (1, 5, 20, 32)  # 73, 402, 1 681 and 2 831 objects; 6, 35, 141 and 235 rooms


def test_batches_reach_the_slab_counts():
    """the docstring's derivation, evaluated: which slab counts the un-pack sums at the four batch sizes"""
    seen = set()
    for n in BATCHES:
        b = workloads.config2_batch(n)
        n_obj, n_room = int(b["objects"].x.size(0)), int(b["rooms"].x.size(0))
        seen |= {tn_slabs(n_obj, 60), tn_slabs(n_room, 6), tn_slabs(n_obj, 9), tn_slabs(n_room, 9)}
    assert {1, 2, 8, 16} <= seen and max(seen) == 16, sorted(seen)
    assert seen & {4, 5, 10}, sorted(seen)  # partial batches of 16 that are no power of two


@pytest.mark.parametrize("n_graphs", BATCHES)
def test_small_batch_sequence_across_the_slab_counts(n_graphs):
    """Adam rides in the un-pack (SAGE, one rank): records of copy segments, 1 .. 16 slabs"""
    ora, batch, ref = sage_case(n_graphs)
    check(ora, SAGE2, batch, ref)


def test_two_rank_shaped_step_runs_unpack_and_adam_apart():
    """force_collective: un-pack without Adam, the (single-rank) all-reduce, then adam_kernel -- the same numbers"""
    ora, batch, ref = sage_case(5)
    check(ora, SAGE2, batch, ref, force_collective=True)


def test_class_weighted_step_divides_by_the_weight_sum():
    """class weights: Adam's normaliser is sum(w[y]) (the gscale path), weights below and above 1"""
    g = torch.Generator().manual_seed(3)
    w = (0.25 + 1.5 * torch.rand(26, generator=g)).tolist()
    ora = pair(SAGE2)
    batch = workloads.config2_batch(5)
    check(ora, SAGE2, batch, oracle_steps(ora, batch, weight=w), weight=w)


@pytest.mark.parametrize("out_dim", [255, 256, 257])
def test_element_counts_around_a_workgroup_and_vectors(out_dim):
    """segments of 255 / 256 / 257 elements with cols = 1 (the last layer's bias vectors: one workgroup less one thread, one full
    workgroup, one workgroup and a second of a single thread), next to 16 x 16 = 256-element and 16 x 6 weight matrices"""
    kw = dict(input_dim_dict={"objects": 16, "rooms": 6}, output_dim=out_dim, conv_block="GraphSAGE", hidden_dim=16, num_layers=2,
              dropout=0.0)
    ora = pair(kw, seed=out_dim)
    batch = workloads.mp3d_like_batch(3, seed=21, sem_dim=10)
    assert any(p.numel() == out_dim and p.dim() == 1 for p in ora.parameters())
    assert any(p.numel() == 256 and p.dim() == 2 for p in ora.parameters())
    check(ora, kw, batch, oracle_steps(ora, batch))


@pytest.mark.parametrize("block", ["GAT", "GAT_edge"])
def test_gat_segments_go_through_the_segment_table(block):
    """2 layers, 2 heads, hidden 8: gradient terms that read parameters (outer products with the attention vectors, the
    wavefront-per-element dot products, three-term segments where lin_dst is lin_src); the un-pack runs without in-kernel Adam"""
    edge = block == "GAT_edge"
    dims = {"objects": 9, "rooms": 3} if edge else {"objects": 12, "rooms": 6}
    kw = dict(input_dim_dict=dims, output_dim=26, conv_block=block, GAT_hidden_dims=[8], GAT_heads=[2, 2], GAT_concats=[True, False],
              dropout=0.0)
    ora = pair(kw, seed=2, bias_noise=True)
    batch = workloads.mp3d_like_batch(4, seed=9, relative_pos=edge, sem_dim=6)
    check(ora, kw, batch, oracle_steps(ora, batch))


def test_linear_heads_sum_more_than_sixteen_slabs():
    """the two-headed homogeneous step: the heads' gradients are one slab per workgroup of the head kernel, ceil(rows / 32) > 16
    here, so the un-pack continues past its first batch of 16.  Phase A of the step (force_collective at lr 0) against
    loss.backward() on a twin, the comparison and tolerances of tests/test_gpu_semisupervised_homog.py::check_against_autograd"""
    data = workloads.stanford_semisupervised_batch(40, 17).to(DEV)
    rows = int(data.x.size(0))
    assert 16 < cdiv(rows, 32) <= 240, rows
    torch.manual_seed(1)
    a = HomogeneousNetwork(input_dim=6, output_dim_dict={"room": 15, "object": 35}, conv_block="GraphSAGE", hidden_dim=32, num_layers=3,
                           dropout=0.0)
    b = copy.deepcopy(a)
    a, b = a.to(DEV), b.to(DEV)
    a.train()
    rm, om, mask = data.room_mask, ~data.room_mask, data.train_mask
    loss = a.loss(a(data), (data.y[rm], data.y[om]), (mask[rm], mask[om]))
    loss.backward()
    step = b.semisupervised_step(lr=0.0, use_graph=False, force_collective=True)
    step(data, mask=mask)
    torch.cuda.synchronize()
    cnt = float(step.grads[b.native().n_active + 1])
    assert abs(step.loss() - float(loss)) <= 2e-5 * max(1.0, abs(float(loss)))
    pb = dict(b.named_parameters())
    seen_heads = 0
    for name, p in a.named_parameters():
        if p.grad is None:
            continue
        off = b.native().param_offsets[id(pb[name])]
        g = step.grads[off: off + p.numel()].view(p.shape) / max(cnt, 1.0)
        torch.testing.assert_close(g, p.grad, atol=2e-5, rtol=1e-4, msg=lambda m: f"{name}: {m}")
        seen_heads += name.startswith("post_mp_")
    assert seen_heads == 4
