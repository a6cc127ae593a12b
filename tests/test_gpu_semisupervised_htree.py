"""Fused step of the two-headed task on the heterogeneous Neural-Tree network: ``HeterogeneousNeuralTreeNetwork(output_dim_dict=...)
.semisupervised_step`` runs the loop body of the reference's ``SemiSupervisedTrainingJob.train`` (semisupervised_training_job.py:
117-147) with each head's CE on the LeafPool of its final state (heterogeneous_neural_tree_network.py:186-205), and ``count_correct``
the per-batch arithmetic of its ``test()`` (:198-257).  The step must equal the ``loss.backward()`` loop on the same engine (same
dropout masks), the oracle in float64, and the data-parallel protocol."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from hydra_gnn_amd import _lib, workloads  # noqa: E402
from hydra_gnn_amd.models import HeterogeneousNeuralTreeNetwork  # noqa: E402
from oracle import models as omodels  # noqa: E402
from test_gpu_semisupervised import LR, WD, launches_of  # noqa: E402

DEV = "cuda:0"
HT_DIMS = {"object": 306, "room": 6, "object-room": 6, "room-room": 6, "object_virtual": 306, "room_virtual": 6}
OUT = {"room": 15, "object": 35, "object-room": 1, "room-room": 1}


def model_kw(block, init=False, dropout=0.25, out=None):
    return dict(input_dim_dict=dict(HT_DIMS), output_dim_dict=dict(out or OUT), conv_block=block, hidden_dim=32, num_layers=3,
                GAT_hidden_dims=[16, 16], GAT_heads=[2, 2, 2], GAT_concats=[True, True, False], disable_initialization=not init,
                dropout=dropout)


def twin_nets(block, init=False, seed=0, **kw):
    """two identical fresh models (same weights, same dropout seed, counters at 0)"""
    torch.manual_seed(seed)
    a = HeterogeneousNeuralTreeNetwork(**model_kw(block, init, **kw))
    b = copy.deepcopy(a)
    return a.to(DEV), b.to(DEV)


def batch_of(block, n=4, seed=13):
    return workloads.semisupervised_htree_batch(n, seed, relative_pos=block == "GAT_edge").to(DEV)


def targets(gb, mask="train_mask"):
    labels = (gb["room_virtual"].y, gb["object_virtual"].y)
    masks = None if mask is None else (getattr(gb["room_virtual"], mask), getattr(gb["object_virtual"], mask))
    return labels, masks


def compare_params(got, ref, tiny, steps, what):
    """test_gpu_semisupervised.compare_params over 8 steps: Adam-ill-conditioned elements (|grad| < 1e-5 at some step) excluded, the
    bulk within 5e-5 (3 % may drift further: the pre_mp GAT layer's elements do after 8 steps), nothing beyond 1e-3 or the travel"""
    n_tiny = n_all = 0
    for name, p in got.named_parameters():
        r = ref[name].detach().cpu().double()
        diff = (p.detach().cpu().double() - r).abs()
        ok = ~tiny[name]
        n_tiny += int(tiny[name].sum())
        n_all += tiny[name].numel()
        if bool(ok.any()):
            assert float(diff[ok].max()) <= 1e-3, f"{name} ({what})"
            assert float((diff[ok] > 5e-5).double().mean()) < 0.03, f"{name} ({what})"
        assert float(diff.max()) <= steps * LR * 2.1, f"{name} ({what})"
    # (the H-tree GAT nets' attention and deep-layer gradients are small: over 8 steps about 45 % of their elements fall under 1e-5
    # at some step; those are still held to the travel bound above)
    assert n_tiny < 0.5 * n_all


CASES = [("GraphSAGE", False), ("GAT", False), ("GAT_edge", False), ("GraphSAGE", True)]


@pytest.mark.parametrize("block,init", CASES)
def test_fused_step_equals_autograd_loop(block, init):
    """path A: net(batch) -> net.loss -> backward -> torch.optim.Adam; path B: semisupervised_step, eager and graph-replayed, 8 steps.
    The last-layer convs into object-room / room-room feed nothing: autograd leaves their .grad None, Adam (weight decay included)
    leaves them alone, and so must the fused step"""
    gb = batch_of(block)
    labels, masks = targets(gb)
    a, _ = twin_nets(block, init)
    init_params = {n: p.detach().clone() for n, p in a.named_parameters()}
    opt = torch.optim.Adam(a.parameters(), lr=LR, weight_decay=WD)
    tiny = {n: torch.zeros_like(p, dtype=torch.bool, device="cpu") for n, p in a.named_parameters()}
    a.train()
    losses_a = []
    for _ in range(8):
        opt.zero_grad()
        loss = a.loss(a(gb), labels, masks)
        loss.backward()
        for n, p in a.named_parameters():
            if p.grad is not None:
                tiny[n] |= (p.grad.abs() < 1e-5).cpu()
        opt.step()
        losses_a.append(float(loss))
    dead = [n for n, p in a.named_parameters() if p.grad is None]
    last = f"convs.{a.num_layers - 1}.convs."
    unused = [n for n in dead if n.startswith(last)]  # (GAT also leaves lin_dst of same-type convs unused: SURVEY A.3 item 1)
    assert unused and all(n[len(last):].split(".")[0].split("__")[2] in ("object-room", "room-room") for n in unused), unused
    assert all(p.grad is None for n, p in a.named_parameters()
               if n.startswith(last) and n[len(last):].split(".")[0].split("__")[2] in ("object-room", "room-room"))
    ref = dict(a.named_parameters())
    for use_graph in (False, True):
        _, b = twin_nets(block, init)
        step = b.semisupervised_step(lr=LR, weight_decay=WD, use_graph=use_graph)
        losses_b = []
        for _ in range(8):
            step(gb, labels, masks)
            losses_b.append(step.loss())
        np.testing.assert_allclose(losses_b, losses_a, rtol=2e-5, atol=2e-6)
        compare_params(b, ref, tiny, 8, f"{block}, init={init}, graph={use_graph}")
        got = dict(b.named_parameters())
        for n in dead:
            assert torch.equal(got[n].detach(), init_params[n]), n
        assert b.native().read_state() == (8, 0)


def test_fused_step_gradient_matches_oracle():
    """SAGE, dropout 0.25: the flat gradient of one fused step / count == oracle.models.HeterogeneousNeuralTreeNetwork in float64
    with the keep-masks (hidden layers and the tail, on the leaf rows) replayed through hmp_dropout_mask at step 1"""
    torch.manual_seed(4)
    kw = model_kw("GraphSAGE", dropout=0.25)
    ora = omodels.HeterogeneousNeuralTreeNetwork(**kw)
    net = HeterogeneousNeuralTreeNetwork(**kw)
    net.load_state_dict(ora.state_dict(), strict=True)
    net = net.to(DEV)
    gb = batch_of("GraphSAGE", 4, seed=5)
    labels, masks = targets(gb)
    lib = _lib.require_device()

    def replay(x, p, training, tag):
        if not training or p == 0:
            return x
        layer, t = tag[1:].split(".", 1)
        n, f = x.shape
        m = torch.zeros(max(n * f, 1), dtype=torch.uint8, device=DEV)
        if n * f:
            _lib.check(lib.hmp_dropout_mask(net._seed, 1, net._drop_stream(int(layer), t), p, n, f, m.data_ptr(), _lib.stream_ptr()))
        return x * m[: n * f].view(n, f).cpu().to(x.dtype) / (1.0 - p)

    o64 = copy.deepcopy(ora).double().train()
    o64.dropout_fn = replay
    b64 = gb.to("cpu")
    for t in b64.node_types:
        if "x" in b64[t]:
            b64[t].x = b64[t].x.double()
    loss = o64.loss(o64(b64), tuple(y.cpu() for y in labels), tuple(m.cpu() for m in masks))
    loss.backward()
    step = net.semisupervised_step(lr=0.0, use_graph=False, force_collective=True)
    step(gb, labels, masks)
    torch.cuda.synchronize()
    nn_ = net.native()
    count = float(step.grads[nn_.n_active + 1])
    assert count == float(masks[0].sum() + masks[1].sum())
    assert abs(step.loss() - float(loss)) <= 1e-5 * max(1.0, abs(float(loss)))
    og = dict(o64.named_parameters())
    for name, p in net.named_parameters():
        ref = og[name].grad
        off = nn_.param_offsets[id(p)]
        if ref is None:
            assert off >= nn_.n_active, name
            continue
        g = step.grads[off:off + p.numel()].view(p.shape).cpu().double() / count
        torch.testing.assert_close(g, ref, atol=1e-5, rtol=1e-5, msg=lambda m: f"{name}: {m}")


def autograd_one_step(a, gb, labels, masks):
    """the reference loss (summed CE of both pooled heads over one count) and its gradients, through the op-by-op forward"""
    a.train()
    pr, po = a(gb)
    lsum = pr.sum() * 0.0
    count = 0
    for p, y, m in zip((pr, po), labels, masks):
        if int(m.sum()) > 0:
            lsum = lsum + F.cross_entropy(p[m], y[m], reduction="sum")
            count += int(m.sum())
    loss = lsum / count
    loss.backward()
    return float(loss), count


def fused_one_step(b, gb, labels, masks):
    """phase A only (force_collective without a process group: A, no-op all-reduce, B at lr 0): flat gradient sums + tail"""
    step = b.semisupervised_step(lr=0.0, use_graph=False, force_collective=True)
    step(gb, labels, masks)
    torch.cuda.synchronize()
    return step


def check_edge_case(a, b, gb, labels, masks):
    loss, count = autograd_one_step(a, gb, labels, masks)
    step = fused_one_step(b, gb, labels, masks)
    nn_ = b.native()
    assert float(step.grads[nn_.n_active + 1]) == count
    assert abs(step.loss() - loss) <= 2e-5 * max(1.0, abs(loss))
    for (name, p_ref), p in zip(a.named_parameters(), b.parameters()):
        off = nn_.param_offsets[id(p)]
        if p_ref.grad is None:
            assert off >= nn_.n_active, name
            continue
        g = step.grads[off:off + p.numel()].view(p.shape) / count
        torch.testing.assert_close(g, p_ref.grad, atol=1e-6, rtol=1e-4, msg=lambda m: f"{name}: {m}")


def edited_pool_batch(block="GraphSAGE"):
    """room_virtual row 0 loses its leaves (so those leaves have no pool edge), room leaf 0 gains a second pool edge (to
    room_virtual row 1), object_virtual row 2 loses its leaves; all three virtual rows are in the train mask"""
    gb = batch_of(block, 2, seed=29)
    et = ("room", "r_to_rv", "room_virtual")
    ei = gb[et].edge_index
    keep = ei[1] != 0
    assert int((~keep).sum()) > 0
    extra = torch.tensor([[int(ei[0, keep][0])], [1]], dtype=torch.int64, device=DEV)
    gb[et].edge_index = torch.cat([ei[:, keep], extra], 1).contiguous()
    et = ("object", "o_to_ov", "object_virtual")
    ei = gb[et].edge_index
    gb[et].edge_index = ei[:, ei[1] != 2].contiguous()
    for t, rows in (("room_virtual", (0, 1)), ("object_virtual", (2,))):
        for r in rows:
            gb[t].train_mask[r] = True
    return gb


@pytest.mark.parametrize("block", ["GraphSAGE", "GAT"])
def test_edge_cases_empty_row_unpooled_leaf_two_edges(block):
    gb = edited_pool_batch(block)
    labels, masks = targets(gb)
    a, b = twin_nets(block)
    check_edge_case(a, b, gb, labels, masks)


def test_all_false_mask_drops_that_head():
    gb = batch_of("GraphSAGE")
    labels, masks = targets(gb)
    masks = (masks[0], torch.zeros_like(masks[1]))
    a, b = twin_nets("GraphSAGE")
    check_edge_case(a, b, gb, labels, masks)


def test_batch_without_object_virtual_rows():
    gb = batch_of("GraphSAGE", 2, seed=31)
    gb["object_virtual"].x = gb["object_virtual"].x[:0].contiguous()
    for k in ("y", "train_mask", "val_mask", "test_mask"):
        setattr(gb["object_virtual"], k, getattr(gb["object_virtual"], k)[:0].contiguous())
    et = ("object", "o_to_ov", "object_virtual")
    gb[et].edge_index = gb[et].edge_index[:, :0].contiguous()
    assert int(gb["object_virtual"].num_nodes) == 0 and int(gb["object"].num_nodes) > 0
    labels, masks = targets(gb)
    a, b = twin_nets("GraphSAGE")
    check_edge_case(a, b, gb, labels, masks)


def test_seventy_object_classes():
    """70 classes: more than one quad per lane in the pooled CE and the leaf gradient"""
    gb = batch_of("GraphSAGE", 2, seed=37)
    g = torch.Generator().manual_seed(3)
    gb["object_virtual"].y = torch.randint(0, 70, (int(gb["object_virtual"].num_nodes),), generator=g).to(DEV)
    labels, masks = targets(gb)
    a, b = twin_nets("GraphSAGE", out=dict(OUT, object=70))
    check_edge_case(a, b, gb, labels, masks)


def test_out_of_range_label_sets_status_bit():
    gb = batch_of("GraphSAGE", 2)
    labels, masks = targets(gb)
    yo = labels[1].clone()
    yo[int(torch.nonzero(masks[1])[0])] = 35
    _, b = twin_nets("GraphSAGE")
    step = fused_one_step(b, gb, (labels[0], yo), masks)
    assert b.native().read_state()[1] & 2
    with pytest.raises(_lib.HydraMPError):
        step.loss()


def reference_test_counts(net, gb, mask_name):
    """the reference's test() per batch, in torch on the eval-mode pooled rows"""
    net.eval()
    with torch.no_grad():
        pred = [p.argmax(dim=1) for p in net(gb)]
    labels, masks = targets(gb, mask_name)
    out = []
    for p, l, m in zip(pred, labels, masks):
        out += [int(p[m].eq(l[m]).sum()), int(torch.numel(l[m]))]
    return out


@pytest.mark.parametrize("block", ["GraphSAGE", "GAT_edge"])
def test_count_correct_matches_reference_test(block):
    """four batches accumulated into ONE device tensor (read once at the end) == the reference's arithmetic summed"""
    net, _ = twin_nets(block)
    batches = [batch_of(block, 2, seed=41 + k) for k in range(4)]
    for mask_name in ("train_mask", "val_mask", "test_mask"):
        want = [0, 0, 0, 0]
        for gb in batches:
            want = [w + v for w, v in zip(want, reference_test_counts(net, gb, mask_name))]
        acc = torch.zeros(4, dtype=torch.int64, device=DEV)
        for gb in batches:
            labels, masks = targets(gb, mask_name)
            assert net.count_correct(gb, labels, masks, counts=acc) is acc
        assert acc.tolist() == want, (block, mask_name)
        assert want[1] > 0 and want[3] > 0


def test_count_correct_empty_rows_and_ties():
    """a virtual row without leaves pools to 0 (argmax 0); every room logit negative: ReLU zeroes the rows, the first index wins"""
    gb = edited_pool_batch()
    net, _ = twin_nets("GraphSAGE")
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.startswith(f"convs.{net.num_layers - 1}.") and name.endswith("__room.lin_l.bias"):
                p.add_(-1e3)
    for mask_name in ("train_mask", "test_mask"):
        labels, masks = targets(gb, mask_name)
        assert net.count_correct(gb, labels, masks) == reference_test_counts(net, gb, mask_name)
    net.eval()
    with torch.no_grad():
        pr, _ = net(gb)
    assert bool((pr == 0).all())


def test_bitwise_deterministic():
    gb = batch_of("GAT", 4, seed=43)
    labels, masks = targets(gb)
    flats = []
    for _ in range(2):
        _, b = twin_nets("GAT", seed=9)
        step = b.semisupervised_step(lr=LR, weight_decay=WD, use_graph=False)
        for _ in range(5):
            step(gb, labels, masks)
        torch.cuda.synchronize()
        flats.append(b.native().flat_params().clone())
    assert torch.equal(flats[0], flats[1])


@pytest.mark.parametrize("block", ["GraphSAGE", "GAT"])
def test_launch_structure(block):
    """the two-head step issues at most one launch more than the single-output H-tree train_step of the same architecture: the
    pooled CE and the leaf gradient replace its pool forward, masked_ce_rows and pool backward"""
    gb = batch_of(block, 16, seed=21)
    torch.manual_seed(0)
    kw = model_kw(block)
    two = HeterogeneousNeuralTreeNetwork(**kw).to(DEV)
    kw.pop("output_dim_dict")
    one = HeterogeneousNeuralTreeNetwork(output_dim=15, **kw).to(DEV)
    labels, masks = targets(gb)
    n_two = launches_of(two, two.semisupervised_step(lr=LR, use_graph=False), gb, labels, masks)
    n_one = launches_of(one, one.train_step(lr=LR, ignored_label=25, use_graph=False), gb, gb["room_virtual"].y)
    assert n_two <= n_one + 1, (n_two, n_one)


@pytest.mark.parametrize("block", ["GraphSAGE", "GAT"])
def test_collective_path_equals_fused_path(block):
    """one rank, force_collective=True (phase A, all-reduce, phase B) == the single fused call"""
    gb = batch_of(block, 4, seed=47)
    labels, masks = targets(gb)
    a, b = twin_nets(block, seed=3)
    sa = a.semisupervised_step(lr=LR, weight_decay=WD, use_graph=False)
    sb = b.semisupervised_step(lr=LR, weight_decay=WD, use_graph=False, force_collective=True)
    for _ in range(3):
        sa(gb, labels, masks)
        sb(gb, labels, masks)
        assert abs(sa.loss() - sb.loss()) <= 1e-6 * max(1.0, abs(sa.loss()))
    torch.testing.assert_close(a.native().flat_params(), b.native().flat_params(), atol=1e-6, rtol=1e-5)
