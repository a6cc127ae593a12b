"""State that must survive what a real training loop does between steps:

* a shuffled DataLoader delivers batches of varying size, so the workspace is re-bound mid-training: Adam's ``t``, the dropout
  draw number and the status bits must not restart (``base_training_job.py:202-216`` + ``torch.optim.Adam`` semantics);
* Adam's ``t`` belongs to the optimiser (``state['step']``), not to the network: a second ``TrainStep`` starts at ``t = 1``;
* ``StepLR`` (``base_training_job.py:186-188``) changes the rate between epochs: ``TrainStep.set_lr``;
* stale-descriptor and stale-activation hazards of the host side fail loudly / are not there;
* a step the executor refuses leaves no step state behind for the next backward.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hydra_gnn_amd import _lib, workloads  # noqa: E402
from hydra_gnn_amd.data import collate  # noqa: E402
from hydra_gnn_amd.models import HeterogeneousNetwork  # noqa: E402
from oracle import models as omodels  # noqa: E402

DEV = "cuda:0"
KW = dict(input_dim_dict={"objects": 306, "rooms": 6}, output_dim=26, conv_block="GraphSAGE", hidden_dim=64, num_layers=3, dropout=0.0)


def pair(seed=0, **over):
    torch.manual_seed(seed)
    kw = dict(KW, **over)
    ora = omodels.HeterogeneousNetwork(**kw)
    net = HeterogeneousNetwork(**kw)
    net.load_state_dict(ora.state_dict(), strict=True)
    return ora, net.to(DEV)


def to64(batch):
    b = batch.to("cpu")
    for t in b.node_types:
        b[t].x = b[t].x.double()
    return b


def assert_params_track(net, o64, n_steps, lr, what):
    """Adam divides by |g|: elements whose gradient is ~eps are ill-conditioned (see test_gpu_models.py); the bulk of every
    tensor must agree tightly and nothing may be further off than the distance n_steps of size lr can cover."""
    ref = dict(o64.named_parameters())
    for name, p in net.named_parameters():
        d = (p.detach().cpu().double() - ref[name].detach()).abs()
        assert float((d > 5e-5).double().mean()) < 0.02, f"{what}: {name}"
        assert float(d.max()) <= n_steps * lr * 2.1, f"{what}: {name}"


@pytest.mark.parametrize("use_graph", [False, True])
def test_growing_batches_rebind_the_workspace_without_restarting_adam(use_graph):
    ora, net = pair()
    o64 = copy.deepcopy(ora).double()
    lr = 0.002
    opt = torch.optim.Adam(o64.parameters(), lr=lr, weight_decay=0.001)
    step = net.train_step(lr=lr, weight_decay=0.001, ignored_label=25, use_graph=use_graph)
    rng = np.random.default_rng(5)
    graphs = [workloads.mp3d_like_graph(rng) for _ in range(24)]
    sizes = [2, 2, 4, 3, 8, 8, 16, 5, 24, 24]  # capacities grow at steps 2, 4, 6, 8: four re-binds
    losses, losses_ref, rebinds, ws_id = [], [], 0, None
    for it, bs in enumerate(sizes):
        batch = collate(graphs[:bs])
        y = batch["rooms"].y
        step(batch.to(DEV), y.to(DEV))
        losses.append(step.loss())
        if ws_id is not None and id(net.native()._ws) != ws_id:
            rebinds += 1
        ws_id = id(net.native()._ws)
        opt.zero_grad()
        loss = o64.loss(o64(to64(batch)), y, y != 25)
        loss.backward()
        opt.step()
        losses_ref.append(float(loss.detach()))
    assert rebinds >= 3, "the test must force workspace re-binds"
    np.testing.assert_allclose(losses, losses_ref, rtol=5e-5, atol=5e-5)
    assert_params_track(net, o64, len(sizes), lr, f"graph={use_graph}")
    assert step.steps_taken() == len(sizes)
    st, status = net.native().read_state()
    assert st == len(sizes) and status == 0


def test_status_bits_survive_a_rebind():
    _, net = pair()
    step = net.train_step(lr=0.002, ignored_label=25, use_graph=False)
    rng = np.random.default_rng(6)
    graphs = [workloads.mp3d_like_graph(rng) for _ in range(8)]
    small = collate(graphs[:2])
    y = small["rooms"].y.clone()
    y[0] = 999  # label out of range: status bit 1
    step(small.to(DEV), y.to(DEV))
    assert net.native().read_state()[1] & 2
    big = collate(graphs)
    step(big.to(DEV), big["rooms"].y.to(DEV))  # larger batch: re-bind
    st, status = net.native().read_state()
    assert st == 2 and (status & 2), "status bits were lost by the workspace re-bind"


def test_second_train_step_on_the_same_net_starts_adam_at_t1():
    ora, net = pair(seed=1)
    batch = workloads.config2_batch(6)
    y = batch["rooms"].y
    gb, yg = batch.to(DEV), y.to(DEV)
    o64 = copy.deepcopy(ora).double()
    b64 = to64(batch)
    lr = 0.002

    def ref_steps(n):
        opt = torch.optim.Adam(o64.parameters(), lr=lr, weight_decay=0.001)  # fresh optimiser state, warm parameters
        for _ in range(n):
            opt.zero_grad()
            o64.loss(o64(b64), y, y != 25).backward()
            opt.step()

    s1 = net.train_step(lr=lr, weight_decay=0.001, ignored_label=25, use_graph=False)
    for _ in range(7):
        s1(gb, yg)
    ref_steps(7)
    s2 = net.train_step(lr=lr, weight_decay=0.001, ignored_label=25, use_graph=False)  # as bench.py's profiling leg does
    for _ in range(3):
        s2(gb, yg)
    ref_steps(3)
    assert s1.steps_taken() == 7 and s2.steps_taken() == 3
    assert_params_track(net, o64, 10, lr, "second optimiser")
    # with t carried over from s1 the bias correction of the first s2 step would be ~(1 - 0.9^8) instead of 0.1: the very first
    # update would be ~5.7x too small -- caught by the tight bulk criterion above


def test_set_lr_follows_a_scheduler():
    """StepLR(step_size=2, gamma=0.5) around the native step == torch's scheduler around torch.optim.Adam."""
    for use_graph in (False, True):
        ora, net = pair(seed=2)
        batch = workloads.config2_batch(6)
        y = batch["rooms"].y
        gb, yg = batch.to(DEV), y.to(DEV)
        o64 = copy.deepcopy(ora).double()
        b64 = to64(batch)
        opt = torch.optim.Adam(o64.parameters(), lr=0.004, weight_decay=0.001)
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.5)
        step = net.train_step(lr=0.004, weight_decay=0.001, ignored_label=25, use_graph=use_graph)
        for epoch in range(6):
            step.set_lr(sched.get_last_lr()[0])
            step(gb, yg)
            opt.zero_grad()
            o64.loss(o64(b64), y, y != 25).backward()
            opt.step()
            sched.step()
        assert_params_track(net, o64, 6, 0.004, f"StepLR graph={use_graph}")
        # a constant-rate run must NOT match (the schedule really was applied)
        _, net_c = pair(seed=2)
        step_c = net_c.train_step(lr=0.004, weight_decay=0.001, ignored_label=25, use_graph=use_graph)
        for _ in range(6):
            step_c(gb, yg)
        far = 0
        for (_, a), (_, b) in zip(net.named_parameters(), net_c.named_parameters()):
            far += int(((a - b).abs() > 1e-3).sum())
        assert far > 100


def test_absent_edge_type_is_refused_and_empty_is_accepted():
    ora, net = pair(seed=3)
    batch = workloads.config2_batch(3)
    et = ("rooms", "rooms_to_rooms", "rooms")
    # present but empty: accepted, equals the oracle (PyG runs the conv: root + bias only)
    batch[et].edge_index = torch.zeros(2, 0, dtype=torch.int64)
    net.eval(); ora.eval()
    out = net(batch.to(DEV))
    torch.testing.assert_close(out.cpu().double(), copy.deepcopy(ora).double()(to64(batch)).detach(), atol=1e-5, rtol=1e-5)

    class NoRR:  # the hetero accessors without that key (PyG's HeteroConv would skip the conv: a different result)
        def __init__(self, d):
            self.d = d
            self.x_dict = d.x_dict
            self.edge_index_dict = {k: v for k, v in d.edge_index_dict.items() if k != et}

        def __getitem__(self, k):
            return self.d[k]

    with pytest.raises(_lib.HydraMPError, match="no entry"):
        net(NoRR(batch.to(DEV)))


def test_backward_after_a_train_step_fails_loudly():
    _, net = pair(seed=4)
    b1 = workloads.config2_batch(3).to(DEV)
    b2 = workloads.config2_batch(5).to(DEV)
    net.train()
    out = net(b1)
    step = net.train_step(lr=0.002, ignored_label=25, use_graph=False)
    step(b2, b2["rooms"].y)  # overwrites the activations (and re-binds: b2 is larger)
    y = b1["rooms"].y
    with pytest.raises(_lib.HydraMPError, match="LAST forward"):
        net.loss(out, y, y != 25).backward()


def test_converted_inputs_are_not_cached_across_steps():
    """float64 features (the reference's double_precision data) are converted to a private fp32 copy: an in-place edit of
    the caller's tensor between two steps must reach the second step."""
    _, net_a = pair(seed=5)
    _, net_b = pair(seed=5)
    batch = workloads.config2_batch(4)
    y = batch["rooms"].y.to(DEV)
    ga = batch.to(DEV)
    for t in ga.node_types:
        ga[t].x = ga[t].x.double()
    sa = net_a.train_step(lr=0.002, ignored_label=25, use_graph=False)
    sa(ga, y)
    ga["objects"].x.mul_(0.5)  # in place: no mutation stamp, same object ids
    sa(ga, y)
    gb = batch.to(DEV)
    sb = net_b.train_step(lr=0.002, ignored_label=25, use_graph=False)
    sb(gb, y)
    gb2 = batch.to(DEV)
    gb2["objects"].x = gb2["objects"].x * 0.5
    sb(gb2, y)
    assert abs(sa.loss() - sb.loss()) < 1e-6
    for (n, a), (_, b) in zip(net_a.named_parameters(), net_b.named_parameters()):
        assert torch.equal(a, b), n


def test_refused_step_leaves_the_forwards_dropout_to_its_backward():
    """A training step the executor refuses (here: n_out off by one) must leave no state of its own behind: the autograd backward
    of the training-mode forward before it draws that forward's dropout masks, not masks numbered by the refused step's
    optimiser counter.  GAT: its backward replays the attention-dropout draw (feature dropout reads its keep bits back from the
    stored activations)."""
    batch = workloads.config2_batch(4)
    gb = batch.to(DEV)
    y = gb["rooms"].y

    def grads(refused_step):
        torch.manual_seed(7)
        net = HeterogeneousNetwork(input_dim_dict={"objects": 306, "rooms": 6}, output_dim=26, dropout=0.25, conv_block="GAT",
                                   GAT_hidden_dims=[32, 32], GAT_heads=[2, 2, 2], GAT_concats=[True, True, False]).to(DEV)
        net.train()
        out = net(gb)
        if refused_step:
            nat = net.native()
            h = nat.make_batch(gb, y)
            bad = type(h.c).from_buffer_copy(h.c)
            bad.n_out += 1
            ctr = torch.full((4,), 1000, dtype=torch.int32, device=DEV)  # far from the forward's draw number (1)
            g = torch.zeros(nat.n_params + 4, dtype=torch.float32, device=DEV)
            args = _lib.TrainArgs(0.002, 0.9, 0.999, 1e-8, 0.0, 25, net._seed, 1)
            args.d_step = ctr.data_ptr()
            rc = nat._lib.hmp_net_step_fwd_bwd(nat._handle, C.byref(bad), nat.flat_params(full_check=False).data_ptr(),
                                               g.data_ptr(), C.byref(args), _lib.stream_ptr())
            assert rc != 0, "the step must refuse a batch whose n_out is off by one"
        net.loss(out, y, y != 25).backward()
        torch.cuda.synchronize()
        return {n: p.grad.detach().cpu() for n, p in net.named_parameters() if p.grad is not None}

    ref, got = grads(False), grads(True)
    assert ref.keys() == got.keys() and ref
    for n in ref:
        assert torch.equal(ref[n], got[n]), n
