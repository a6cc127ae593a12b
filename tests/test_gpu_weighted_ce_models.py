"""Class-weighted cross entropy at step level, one small batch per model class: the single-head step with the CE riding in the last
aggregation's epilogue (HeterogeneousNetwork GraphSAGE at every row-group size the epilogue is instantiated for: last-layer widths
26 / 40 / 100 / 200 -> 8 / 16 / 32 / 64 lanes per row) and on its own (GAT: masked_ce_rows), the two-headed heterogeneous step
(tails in the epilogue for GraphSAGE, the stand-alone tail launch for GAT), the pooled heads of the H-tree net, the linear heads of
the homogeneous nets, and the GCN op path (net.loss(..., weight=)).

For each: (1) weights all 1.0 and (5) set_class_weight(None) after set_class_weight(w) give the unweighted step's bits --
parameters, Adam moments and the {loss_sum, count} pair; (2) weights all 0.25 with 3 valid rows (weight sum 0.75): the pair is 0.25 x
the unweighted pair and parameters and moments are bit-identical (the backward is linear in the loss gradient and a power of two
scales exactly; Adam divides by 0.75, not by a count clamped to 1); (3) a class of weight 0 == that class's labels ignored; (4) five
steps against the op-level restatement forward -> model.loss(..., weight=w) -> backward -> torch.optim.Adam with the tolerances the
existing step-vs-autograd tests of the model class use (two-headed: losses rtol 2e-5 / atol 2e-6 and their compare_params; single
head: rtol 2e-5 / atol 2e-5 and the same parameter scheme, without dropout, as tests/test_gpu_models.py); (6) a BatchStream
batch steps to the same bits as the host-collated batch.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import test_gpu_semisupervised as t_het  # noqa: E402  (compare_params, LR, WD of the heterogeneous two-head step tests)
import test_gpu_semisupervised_stream as ss  # noqa: E402  (graphs, models and host steps of the four two-headed shapes)
from hydra_gnn_amd import workloads  # noqa: E402
from hydra_gnn_amd.data import collate  # noqa: E402
from hydra_gnn_amd.models import HeterogeneousNetwork, HomogeneousNetwork  # noqa: E402
from hydra_gnn_amd.store import GraphStore  # noqa: E402

DEV = "cuda:0"
LR, WD = t_het.LR, t_het.WD
GAT3 = ss.GAT3


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def state_of(step):
    """what a step leaves behind: parameters, Adam moments, {loss_sum, count}"""
    na = step.net.n_active
    torch.cuda.synchronize()
    return [step.flat.clone(), step.m.clone(), step.v.clone(), step.grads[na:na + 2].clone()]


def same_state(a, b, what, pair=True):
    for x, y, name in list(zip(a, b, ("parameters", "m", "v", "pair")))[:4 if pair else 3]:
        assert torch.equal(bits(x), bits(y)), f"{what}: {name} differ"


def rand_w(c, seed):
    return (torch.rand(c, generator=torch.Generator().manual_seed(seed)) * 3.0 + 0.05).float()


# ---- single-head room task -------------------------------------------------------------------------------------------------------
def room_graphs(n=3, seed=5):
    rng = np.random.default_rng(seed)
    return [workloads.mp3d_like_graph(rng) for _ in range(n)]


def room_net(block, out_dim, dropout=0.25):
    torch.manual_seed(0)
    kw = dict(input_dim_dict={"objects": 306, "rooms": 6}, output_dim=out_dim, conv_block=block, hidden_dim=32, num_layers=3,
              dropout=dropout)
    if block != "GraphSAGE":
        kw.update(GAT3)
    return HeterogeneousNetwork(**kw).to(DEV).train()


def room_labels(gb, out_dim, keep=None):
    """labels over all out_dim classes (the generator draws 26), class out_dim - 1 ignored; keep: only these rows stay valid"""
    n = gb["rooms"].y.numel()
    y = torch.randint(0, out_dim, (n,), generator=torch.Generator().manual_seed(n + out_dim)).to(DEV)
    if keep is not None:
        m = torch.zeros(n, dtype=torch.bool, device=DEV)
        m[keep] = True
        y = torch.where(m, y.clamp(max=out_dim - 2), torch.full_like(y, out_dim - 1))
    return y


ROOM_CASES = [("GraphSAGE", 26), ("GraphSAGE", 40), ("GraphSAGE", 100), ("GraphSAGE", 200), ("GAT", 26)]


@pytest.mark.parametrize("block,out_dim", ROOM_CASES)
def test_room_step(block, out_dim):
    graphs = room_graphs()
    gb = collate(graphs).to(DEV)
    ignored = out_dim - 1
    y = room_labels(gb, out_dim)

    def one(weight, labels=y, after=None):
        net = room_net(block, out_dim)
        step = net.train_step(lr=LR, weight_decay=WD, ignored_label=ignored, use_graph=False, class_weight=weight)
        if after is not None:
            after(step)
        step(gb, labels)
        assert net.native().read_state() == (1, 0)
        return state_of(step)

    base = one(None)
    same_state(one([1.0] * out_dim), base, "weights 1.0")                                             # 1
    same_state(one(rand_w(out_dim, 1), after=lambda s: s.set_class_weight(None)), base, "set_class_weight(None)")  # 5
    y3 = room_labels(gb, out_dim, keep=[0, 1, y.numel() - 1])                                          # 2
    b3, q3 = one(None, y3), one(torch.full((out_dim,), 0.25), y3)
    assert b3[3].tolist()[1] == 3.0 and q3[3].tolist()[1] == 0.75
    assert torch.equal(bits(q3[3]), bits(b3[3] * 0.25))
    same_state(q3, b3, "weights 0.25, 3 valid rows", pair=False)
    z = int(y[0]) if int(y[0]) != ignored else 0                                                       # 3
    wz = torch.ones(out_dim)
    wz[z] = 0.0
    same_state(one(wz), one(None, torch.where(y == z, torch.full_like(y, ignored), y)), "class of weight 0")
    zero = one(torch.zeros(out_dim))                                                                   # all weights 0
    assert zero[3].tolist() == [0.0, 0.0] and all(bool(torch.isfinite(t).all()) for t in zero)
    # 4: five steps against forward -> loss(weight=) -> backward -> Adam.  Without dropout, as the single-head step-vs-reference test
    # (tests/test_gpu_models.py::test_fused_train_step_matches_oracle_adam, whose tolerances these are): train_step draws its masks
    # from its own seed argument, not from the module's
    w = rand_w(out_dim, 2).to(DEV)
    a = room_net(block, out_dim, dropout=0.0)
    opt = torch.optim.Adam(a.parameters(), lr=LR, weight_decay=WD)
    tiny = {n: torch.zeros_like(p, dtype=torch.bool, device="cpu") for n, p in a.named_parameters()}
    losses_a = []
    for _ in range(5):
        opt.zero_grad()
        loss = a.loss(a(gb), y, y != ignored, weight=w)
        loss.backward()
        for n, p in a.named_parameters():
            if p.grad is not None:
                tiny[n] |= (p.grad.abs() < 1e-5).cpu()
        opt.step()
        losses_a.append(float(loss))
    b = room_net(block, out_dim, dropout=0.0)
    step = b.train_step(lr=LR, weight_decay=WD, ignored_label=ignored, use_graph=True, class_weight=w)
    losses_b = []
    for _ in range(5):
        step(gb, y)
        losses_b.append(step.loss())
    print(f"  {block} {out_dim}: losses {losses_b} (autograd {losses_a})")
    np.testing.assert_allclose(losses_b, losses_a, rtol=2e-5, atol=2e-5)
    t_het.compare_params(b, dict(a.named_parameters()), tiny, 5, f"{block} {out_dim}")
    # the weighted mean is torch's, on the logits of a plain forward
    b.eval()
    pred = b(gb)
    valid = y != ignored
    ref = F.cross_entropy(pred[valid].double().cpu(), y[valid].cpu(), weight=w.double().cpu())
    torch.testing.assert_close(b.loss(pred, y, valid, weight=w).double().cpu(), ref, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("block,out_dim", [("GraphSAGE", 26), ("GAT", 26)])
def test_room_step_on_a_stream_batch(block, out_dim):
    graphs = room_graphs(4, seed=6)
    ids = [2, 0, 3]
    gb = collate([graphs[i] for i in ids]).to(DEV)
    w = rand_w(out_dim, 3)
    net = room_net(block, out_dim)
    step = net.train_step(lr=LR, weight_decay=WD, ignored_label=25, use_graph=False, class_weight=w)
    step(gb, gb["rooms"].y)
    host = state_of(step)
    net = room_net(block, out_dim)
    stream = GraphStore(graphs, DEV).stream(net, 3, "rooms")
    step = net.train_step(lr=LR, weight_decay=WD, ignored_label=25, use_graph=False, class_weight=w)
    step.run(stream.next(ids))
    same_state(state_of(step), host, "stream batch")
    assert host[3].tolist()[1] > 0


# ---- the two-headed shapes -------------------------------------------------------------------------------------------------------
def head_rows(shape, net, gb, mask="train_mask"):
    """per head: (the label vector's owner and name, bool rows of that vector the head counts under `mask`)"""
    if shape.startswith("homog"):
        rm = gb.room_mask
        om = gb.object_mask if shape == "homog_htree" else ~gb.room_mask
        m = getattr(gb, mask)
        return [(gb, rm & m), (gb, om & m)]
    return [(gb[t], getattr(gb[t], mask)) for t in net.native().head_label_types()]


def edit_labels(shape, net, gb, fn):
    """fn(head, y, rows) -> new y, applied head by head to the batch's label vectors"""
    for h, (owner, rows) in enumerate(head_rows(shape, net, gb)):
        owner.y = fn(h, owner.y.clone(), rows)


TWO_HEAD = [("hetero", "GraphSAGE"), ("hetero", "GAT"), ("hetero_htree", "GraphSAGE"), ("homog", "GraphSAGE"), ("homog_htree", "GAT")]


@pytest.mark.parametrize("shape,block", TWO_HEAD)
def test_two_head_step(shape, block):
    n_graphs = 8 if shape == "homog" else 3  # (Stanford-like graphs have one room each: 8 graphs put 3 rooms under train_mask)
    graphs = ss.graphs_of(shape, n_graphs, seed=21, block=block)
    ids = list(range(n_graphs))

    def fresh():
        return ss.twin_nets(shape, block)[0]

    classes = fresh().native().head_classes()

    def one(weight, edit=None, after=None):
        net = fresh()
        gb = ss.host_batch(shape, graphs, ids)
        if edit is not None:
            edit_labels(shape, net, gb, edit)
        step = net.semisupervised_step(lr=LR, weight_decay=WD, use_graph=False, class_weight=weight)
        if after is not None:
            after(step)
        ss.host_step(shape, net, step, gb, "train_mask")
        assert net.native().read_state() == (1, 0)
        return state_of(step)

    base = one(None)
    assert base[3].tolist()[1] > 3
    same_state(one(tuple([1.0] * c for c in classes)), base, "weights 1.0")                                            # 1
    same_state(one({"rooms": torch.ones(classes[0]), "objects": None}), base, "weights 1.0 on one head")
    ws = tuple(rand_w(c, 7 + i) for i, c in enumerate(classes))
    same_state(one(ws, after=lambda s: s.set_class_weight(None)), base, "set_class_weight(None)")                      # 5

    def three_valid(h, y, rows):  # two room rows and one object row stay, every other label is ignored
        keep = torch.nonzero(rows)[: 2 if h == 0 else 1, 0]
        out = torch.where(rows, torch.full_like(y, -100), y)
        out[keep] = y[keep]
        return out

    b3, q3 = one(None, three_valid), one(tuple(torch.full((c,), 0.25) for c in classes), three_valid)                  # 2
    assert b3[3].tolist()[1] == 3.0 and q3[3].tolist()[1] == 0.75
    assert torch.equal(bits(q3[3]), bits(b3[3] * 0.25))
    same_state(q3, b3, "weights 0.25, 3 valid rows", pair=False)
    gb0 = ss.host_batch(shape, graphs, ids)                                                                            # 3
    zs = [int(owner.y[rows][0]) for owner, rows in head_rows(shape, fresh(), gb0)]
    wz = tuple(torch.ones(c) for c in classes)
    for w_, z in zip(wz, zs):
        w_[z] = 0.0
    same_state(one(wz), one(None, lambda h, y, rows: torch.where(rows & (y == zs[h]), torch.full_like(y, -100), y)), "class of weight 0")
    zero = one(tuple(torch.zeros(c) for c in classes))
    assert zero[3].tolist() == [0.0, 0.0] and all(bool(torch.isfinite(t).all()) for t in zero)
    # 6: the stream batch
    net = fresh()
    stream = GraphStore(graphs, DEV).stream(net, n_graphs)
    step = net.semisupervised_step(lr=LR, weight_decay=WD, use_graph=False, class_weight=ws)
    step.run(stream.next(ids), mask="train_mask")
    same_state(state_of(step), one(ws), "stream batch")
    # 4: five steps against forward -> loss(weight=) -> backward -> Adam
    a = fresh()
    gb = ss.host_batch(shape, graphs, ids)
    wd = tuple(w_.to(DEV) for w_ in ws)
    opt = torch.optim.Adam(a.parameters(), lr=LR, weight_decay=WD)
    tiny = {n: torch.zeros_like(p, dtype=torch.bool, device="cpu") for n, p in a.named_parameters()}
    losses_a = []
    for _ in range(5):
        opt.zero_grad()
        if shape.startswith("homog"):
            rows = [gb.room_mask, gb.object_mask if shape == "homog_htree" else ~gb.room_mask]
            labels, masks = tuple(gb.y[r] for r in rows), tuple(gb.train_mask[r] for r in rows)
        else:
            types = a.native().head_label_types()
            labels, masks = tuple(gb[t].y for t in types), tuple(gb[t].train_mask for t in types)
        loss = a.loss(a(gb), labels, masks, weight=wd)
        loss.backward()
        for n, p in a.named_parameters():
            if p.grad is not None:
                tiny[n] |= (p.grad.abs() < 1e-5).cpu()
        opt.step()
        losses_a.append(float(loss))
    b = fresh()
    step = b.semisupervised_step(lr=LR, weight_decay=WD, use_graph=True, class_weight=wd)
    losses_b = []
    for _ in range(5):
        ss.host_step(shape, b, step, gb, "train_mask")
        losses_b.append(step.loss())
    print(f"  {shape} {block}: losses {losses_b} (autograd {losses_a})")
    np.testing.assert_allclose(losses_b, losses_a, rtol=2e-5, atol=2e-6)
    if shape == "hetero_htree":
        import test_gpu_semisupervised_htree as t_ht

        t_ht.compare_params(b, dict(a.named_parameters()), tiny, 5, f"{shape} {block}")
    else:
        t_het.compare_params(b, dict(a.named_parameters()), tiny, 5, f"{shape} {block}")
    # the list form is one weighted sum over one weight sum, torch's own per head
    a.eval()
    pred = a(gb)
    num = den = 0.0
    for p, l, m, w_ in zip(pred, labels, masks, ws):
        v = m & (l != -100)
        num += float(F.cross_entropy(p[v].double().cpu(), l[v].cpu(), weight=w_.double(), reduction="sum"))
        den += float(w_.double()[l[v].cpu()].sum())
    torch.testing.assert_close(float(a.loss(pred, labels, masks, weight=wd)), num / den, atol=1e-5, rtol=1e-5)


# ---- refusals by name --------------------------------------------------------------------------------------------------------------
def test_refusals():
    from hydra_gnn_amd._lib import HydraMPError

    net = room_net("GraphSAGE", 26)
    step = net.train_step(lr=LR, use_graph=False)
    with pytest.raises(HydraMPError, match="wrong length"):
        step.set_class_weight([1.0] * 25)
    with pytest.raises(HydraMPError, match="negative"):
        step.set_class_weight([1.0] * 25 + [-0.5])
    two = ss.twin_nets("hetero")[0]
    s2 = two.semisupervised_step(lr=LR, use_graph=False)
    with pytest.raises(HydraMPError, match="pair"):
        s2.set_class_weight(torch.ones(26))
    with pytest.raises(HydraMPError, match="rooms"):
        s2.set_class_weight({"room_virtual": torch.ones(26)})
    with pytest.raises(HydraMPError, match=r"class_weight\[objects\].*wrong length"):
        s2.set_class_weight((torch.ones(26), torch.ones(26)))
    # the library names both numbers
    gb = collate(room_graphs()).to(DEV)
    step(gb, gb["rooms"].y)
    nat = net.native()
    w = torch.ones(25, device=DEV)
    assert nat._lib.hmp_net_set_class_weights(nat._handle, 0, w.data_ptr(), 25) != 0
    assert b"25 weights for head 0, which has 26 classes" in nat._lib.hmp_last_error()
    assert nat._lib.hmp_net_set_class_weights(nat._handle, 1, w.data_ptr(), 25) != 0  # a one-headed net
    assert nat._lib.hmp_net_set_class_weights(nat._handle, 0, None, 0) == 0


# ---- GCN on the op path ------------------------------------------------------------------------------------------------------------
def test_gcn_op_path_loss():
    torch.manual_seed(0)
    net = HomogeneousNetwork(input_dim=6, output_dim=15, conv_block="GCN", hidden_dim=32, num_layers=3, dropout=0.0).to(DEV).train()
    from hydra_gnn_amd.data import collate_homogeneous

    rng = np.random.default_rng(9)
    gb = collate_homogeneous([workloads.stanford_like_graph(rng) for _ in range(3)]).to(DEV)
    C = 15
    label = torch.randint(0, C, (int(gb.room_mask.sum()),), generator=torch.Generator().manual_seed(1)).to(DEV)
    mask = torch.ones_like(label, dtype=torch.bool)
    if label.numel() > 1:
        mask[-1] = False

    def grads(weight, lab=label, m=mask):
        net.zero_grad()
        pred = net(gb)
        pred.retain_grad()
        loss = net.loss(pred, lab, m, weight=weight)
        loss.backward()
        return loss.detach().clone(), pred.grad.clone(), [p.grad.clone() for p in net.parameters() if p.grad is not None], pred.detach()

    base = grads(None)
    one = grads(torch.ones(C))
    assert torch.equal(bits(base[0]), bits(one[0])) and torch.equal(bits(base[1]), bits(one[1]))                       # 1
    z = int(label[0])
    wz = torch.ones(C)
    wz[z] = 0.0
    gz, gi = grads(wz), grads(None, label, mask & (label != z))                                                       # 3
    assert torch.equal(bits(gz[0]), bits(gi[0])) and torch.equal(bits(gz[1]), bits(gi[1]))
    w = rand_w(C, 4)
    got = grads(w)                                                                                                     # 4
    p64 = got[3].double().cpu().requires_grad_(True)
    ref = F.cross_entropy(p64[mask.cpu()], label[mask].cpu(), weight=w.double())
    ref.backward()
    torch.testing.assert_close(got[0].double().cpu(), ref.detach(), atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(got[1].double().cpu(), p64.grad, atol=1e-5, rtol=1e-5)
    assert all(bool(torch.isfinite(g).all()) for g in got[2]) and len(got[2]) > 0
