"""Monte-Carlo dropout uncertainty through the executor: model.predict_mc / predict_with_uncertainty on all four model classes and
both tasks, on host batches and on store.BatchStream descriptors, evaluate.predict_mc and the jobs' predict_mc().

What is compared with what (tests/_mc_reference.py states the bars and the label rule).  The T score sets are the outputs of the
existing training-mode forward, replayed at the steps predict_mc draws at -- model.train(); model._seed = seed; model._rng_step =
first_step + t - 1; model(batch) -- copied to the host and reduced by the float64 restatement.  GIN: the same forward with its
BatchNorm reading the running statistics (ops.batch_norm told `training = False`), which is the contract of predict_mc.  The room
task and the heterogeneous two-headed nets (pooled heads included) run the Monte-Carlo launch on the values forward() returns: the
bars are those of the kernel test.  The homogeneous two-headed nets compute their heads' logits on the VALU where forward() uses the
MFMA GEMM; at F = 32 the two float32 sums differ by less than the bars notice (measured: mean_probs within 2e-8, entropy and mutual
information within 6e-7 of the reference), so they are held to the same bars with no allowance.  The label rule's cap is taken
over all readout forms of a pass, as the kernel test takes it over its whole list."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _mc_reference import MAX_EXEMPT, check_mc, entropy_tol, mc_reference  # noqa: E402
from hydra_gnn_amd import _lib, evaluate, jobs, ops, workloads  # noqa: E402
from hydra_gnn_amd.data import collate_homogeneous  # noqa: E402
from hydra_gnn_amd.models import HeterogeneousNetwork, HomogeneousNetwork  # noqa: E402
from hydra_gnn_amd.store import GraphStore  # noqa: E402
from test_gpu_predict_models import (CLASS_OF, DEV, KC_LOSS, GraphDataset, ReadCounter, graphs_of, host_batch, launches, opt,  # noqa: E402
                                     room_case, two_head_kw)

SEED = 0x1F2E3D4C5B6A
NAMES = ["sage_room", "hetero_gat", "hetero_gat_edge", "hetero_htree", "homog", "homog_htree", "homog_room", "gcn", "gin"]


def heads_of(result):
    """predict_mc's result as a list of 5-tuples per head"""
    return list(result) if isinstance(result[0], tuple) else [result]


def case(name, dropout=None):
    """(model on the device, three-graph batch on the device, graphs, shape) of a readout form"""
    extra = {} if dropout is None else {"dropout": dropout}
    if name == "sage_room":
        torch.manual_seed(7)
        net = HeterogeneousNetwork({"objects": 306, "rooms": 6}, output_dim=26, conv_block="GraphSAGE", hidden_dim=32, num_layers=3, **extra)
        return net.to(DEV), workloads.mp3d_like_batch(3, seed=19).to(DEV), None, "room"
    if name in ("homog_room", "gcn", "gin"):
        torch.manual_seed(7)
        rng = np.random.default_rng(17)
        block = {"homog_room": "GraphSAGE", "gcn": "GCN", "gin": "GIN"}[name]
        net = HomogeneousNetwork(input_dim=6, output_dim=15, conv_block=block, hidden_dim=16, num_layers=3, **extra)
        if name == "gin":  # running statistics away from (0, 1), so that the BatchNorm mode shows
            with torch.no_grad():
                for bn in net.batch_norms:
                    bn.module.running_mean.uniform_(-0.5, 0.5)
                    bn.module.running_var.uniform_(0.5, 2.0)
        gs = [workloads.stanford_like_graph(rng) for _ in range(10)]
        return net.to(DEV), collate_homogeneous(gs[:3]).to(DEV), gs, "room_node"
    shape, block = {"hetero_gat": ("hetero", "GAT"), "hetero_gat_edge": ("hetero", "GAT_edge"), "hetero_htree": ("hetero_htree", "GraphSAGE"),
                    "homog": ("homog", "GraphSAGE"), "homog_htree": ("homog_htree", "GraphSAGE")}[name]
    kw = two_head_kw(shape, block)
    if name == "hetero_gat_edge":  # relative positions are edge attributes: the node features lose their 3 position columns
        kw["input_dim_dict"] = {"objects": 303, "rooms": 3}
    torch.manual_seed(NAMES.index(name))
    net = CLASS_OF[shape](**kw, **extra)
    with torch.no_grad():  # biases away from 0, so that ReLU rows of zeros are not the rule (two_head_model's lines)
        for pname, p in net.named_parameters():
            if pname.endswith("bias"):
                p.add_(torch.randn_like(p) * 0.2)
    if name == "hetero_gat_edge":
        gs = workloads.semisupervised_graphs(10, 11, relative_pos=True)
    else:
        gs = graphs_of(shape, 10, seed=11 + NAMES.index(name))
    return net.to(DEV), host_batch(shape, gs, [0, 1, 2]), gs, shape


def head_rows(net, shape, batch):
    """per head the node rows of a homogeneous batch (bool, host), None where a head's rows are a whole node type"""
    if shape == "room_node":
        return [batch.room_mask.cpu()]
    if shape.startswith("homog"):
        return [batch.room_mask.cpu(), (batch.object_mask if shape == "homog_htree" else ~batch.room_mask).cpu()]
    return [None] * (2 if shape != "room" else 1)


def replay(net, batch, seed, first_step, T, monkeypatch):
    """per head float32 host scores [T, rows, C] of the existing training-mode forward at the steps predict_mc draws at; the
    module's seed, step counter and training flag are put back"""
    ora, kept = net, (net._seed, net._rng_step, net.training)
    ora.train()
    ora._seed = seed
    if getattr(ora, "conv_block", "") == "GIN":  # BatchNorm on the running statistics, as predict_mc defines its pass
        real = ops.batch_norm
        monkeypatch.setattr(ops, "batch_norm", lambda x, g, b, rm, rv, mom, eps, training: real(x, g, b, rm, rv, mom, eps, False))
    outs = []
    for t in range(T):
        ora._rng_step = first_step + t - 1
        with torch.no_grad():
            out = ora(batch)
        outs.append([o.cpu().numpy() for o in (out if isinstance(out, tuple) else (out,))])
        assert ora._rng_step == first_step + t
    monkeypatch.undo()
    net._seed, net._rng_step = kept[:2]
    net.train(kept[2])
    return [np.stack([o[h] for o in outs]) for h in range(len(outs[0]))]


def check_heads(got, scores, rows, T, tag):
    exempt = compared = 0
    for h, ((lab, mean, sd, ent, mi), s, mem) in enumerate(zip(got, scores, rows)):
        C_ = s.shape[2]
        assert lab.is_cuda and lab.dtype == torch.int64 and all(t.is_cuda and t.dtype == torch.float32 for t in (mean, sd, ent, mi))
        assert all(t.is_contiguous() for t in (lab, mean, sd, ent, mi))
        arrays = [t.cpu().numpy() for t in (lab, mean, sd, ent, mi)]
        ref = mc_reference(s)
        if mem is None:
            e, c = check_mc(arrays, ref, T, C_, f"{tag} head {h}")
        else:  # a row per node: -1 / 0 exactly outside the head's rows
            m = mem.numpy()
            assert (arrays[0][~m] == -1).all() and all((a[~m] == 0).all() for a in arrays[1:])
            e, c = check_mc([a[m] for a in arrays], ref, T, C_, f"{tag} head {h}")
        exempt, compared = exempt + e, compared + c
    return exempt, compared


def state_of(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items()}, net._rng_step, net.training


def same_state(net, before):
    sd, step, training = before
    now = net.state_dict()
    return (net._rng_step, net.training) == (step, training) and set(now) == set(sd) and all(torch.equal(now[k], sd[k]) for k in sd)


# ---- 1. every readout form against the replayed training-mode forward ----------------------------------------------------------------
def forms_against_the_replay(name, first_step, monkeypatch):
    """(rows exempt from the label rule, rows compared) of one readout form over T = 1, 3, 8"""
    net, batch, _, shape = case(name)
    rows = head_rows(net, shape, batch)
    net.eval()
    exempt = compared = 0
    for T in (1, 3, 8):
        before = state_of(net)
        got = heads_of(net.predict_mc(batch, samples=T, seed=SEED, first_step=first_step))
        assert same_state(net, before), f"{name}: predict_mc changed the module"
        scores = replay(net, batch, SEED, first_step, T, monkeypatch)
        assert len(got) == len(scores) == len(rows)
        e, c = check_heads(got, scores, rows, T, f"{name} T {T} first_step {first_step}")
        exempt, compared = exempt + e, compared + c
        again = heads_of(net.predict_mc(batch, samples=T, seed=SEED, first_step=first_step))
        assert all(torch.equal(a, b) for g, w in zip(again, got) for a, b in zip(g, w)), f"{name}: two runs differ"
    print(f"{name}: {exempt} of {compared} rows exempt from the label rule")
    return exempt, compared


@pytest.mark.parametrize("first_step", [1, 1000])
def test_predict_mc_equals_the_reduced_training_mode_forwards(first_step, monkeypatch):
    exempt = compared = 0
    for name in NAMES:
        e, c = forms_against_the_replay(name, first_step, monkeypatch)
        exempt, compared = exempt + e, compared + c
    print(f"first_step {first_step}: {exempt} of {compared} rows exempt from the label rule")
    assert exempt <= MAX_EXEMPT * compared


@pytest.mark.parametrize("name", NAMES)
def test_the_default_seed_is_the_modules_and_the_training_flag_comes_back(name):
    net, batch, _, _ = case(name)
    # seed=None is the module's seed; a training-mode module is handed back in training mode
    net.train()
    before = state_of(net)
    a = heads_of(net.predict_mc(batch, samples=3))
    assert same_state(net, before) and net.training
    b = heads_of(net.predict_mc(batch, samples=3, seed=net._seed, first_step=1))
    assert all(torch.equal(x, y) for g, w in zip(a, b) for x, y in zip(g, w))


# ---- 2. without dropout every sample is the eval-mode forward ------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_without_dropout_predict_mc_is_predict_topk(name):
    net, batch, _, shape = case(name, dropout=0.0)
    net.eval()
    T = 4
    got = heads_of(net.predict_mc(batch, samples=T, seed=SEED))
    top = net.predict_topk(batch, 1)
    top = list(top) if isinstance(top[0], tuple) else [top]
    labels = net.predict_labels(batch)
    labels = list(labels) if isinstance(labels, tuple) else [labels]
    for h, ((lab, mean, sd, ent, mi), (tl, tp), pl) in enumerate(zip(got, top, labels)):
        assert torch.equal(lab, pl) and torch.equal(lab, tl[:, 0]), f"{name} head {h}: labels"
        on = lab >= 0
        conf = mean[on].gather(1, lab[on][:, None])[:, 0]
        assert torch.equal(conf, tp[on][:, 0]), f"{name} head {h}: mean_probs[label] is not the top-1 probability"
        C_ = mean.size(1)
        worst = float(mi.abs().max()) if mi.numel() else 0.0
        print(f"{name} head {h}: largest mutual information of identical samples {worst:.2e} (bar {entropy_tol(T, C_):.2e})")
        assert worst <= entropy_tol(T, C_)
        assert float(sd.max() if sd.numel() else 0.0) <= 2.0 ** -11


# ---- 3. stream descriptors -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sage_room", "hetero_gat", "hetero_htree", "homog", "homog_htree", "homog_room"])
def test_stream_batches_equal_the_host_batch(name):
    if name == "sage_room":
        net, gs, _ = room_case("hetero")
        net, shape = net.to(DEV), "room"
    else:
        net, _, gs, shape = case(name)
    net.eval()
    store = GraphStore(gs, DEV)
    kw = {"label_type": "node"} if shape == "room_node" else {"label_type": "rooms"} if shape == "room" else {}
    stream = store.stream(net, 4, **kw)
    for ids in ([0, 1, 2, 5], [7], [4, 4, 9]):
        got = heads_of(net.predict_mc(stream.next(ids), samples=3, seed=SEED, first_step=5))
        want = heads_of(net.predict_mc(store.collate(ids), samples=3, seed=SEED, first_step=5))
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g[0].numel() > 0 and all(torch.equal(a, b) for a, b in zip(g, w)), (name, ids)
    other = (room_case("hetero")[0].to(DEV) if name == "sage_room" else case(name)[0]).eval()
    with pytest.raises(_lib.HydraMPError, match="another model"):
        other.predict_mc(stream.next([0, 1]), samples=2)


# ---- 4. training is not disturbed -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sage_room", "hetero_gat", "hetero_htree", "homog"])
def test_predict_mc_between_training_steps_leaves_the_losses_bit_equal(name):
    losses = []
    for interleave in (False, True):
        net, batch, _, shape = case(name)
        net.train()
        if shape == "room":
            step = net.train_step(lr=0.01, weight_decay=0.001, ignored_label=25)
            run = lambda: step(batch, batch["rooms"].y)  # noqa: E731
        elif shape.startswith("homog"):
            step = net.semisupervised_step(lr=0.01)
            run = lambda: step(batch)  # noqa: E731
        else:
            step = net.semisupervised_step(lr=0.01)
            types = net.native().head_label_types()
            run = lambda: step(batch, tuple(batch[t].y for t in types), tuple(batch[t].train_mask for t in types))  # noqa: E731
        seq = []
        for _ in range(3):
            run()
            seq.append(step.loss())
            if interleave:
                before = state_of(net)
                net.predict_mc(batch, samples=2)
                assert same_state(net, before)
        losses.append(seq)
    print(name, losses)
    assert losses[0] == losses[1] and all(np.isfinite(v) for v in losses[0])


def test_op_path_models_keep_their_batchnorm_state():
    for name in ("gin", "gcn"):
        net, batch, _, _ = case(name)
        for mode in (False, True):
            net.train(mode)
            before = state_of(net)
            if name == "gin":
                tracked = [int(bn.module.num_batches_tracked) for bn in net.batch_norms]
            net.predict_mc(batch, samples=3)
            net.predict_with_uncertainty(batch, samples=2)
            assert same_state(net, before), (name, mode)
            if name == "gin":
                assert tracked == [int(bn.module.num_batches_tracked) for bn in net.batch_norms]
    torch.manual_seed(3)
    two = HomogeneousNetwork(input_dim=6, output_dim_dict={"room": 15, "object": 35}, conv_block="GCN", hidden_dim=32, num_layers=3).to(DEV).eval()
    batch = host_batch("homog", graphs_of("homog", 4, 15), [0, 1, 2, 3])
    got = heads_of(two.predict_mc(batch, samples=3, seed=SEED))
    rows = head_rows(two, "homog", batch)
    scores = replay(two, batch, SEED, 1, 3, pytest.MonkeyPatch())
    check_heads(got, scores, rows, 3, "homog GCN two-headed")  # hmp_mc_accumulate_rows on forward()'s own logits


# ---- 5. launch budget -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sage_room", "hetero_gat", "hetero_htree", "homog", "homog_htree"])
def test_predict_mc_enqueues_t_training_forwards_plus_a_launch_each_plus_the_finish(name, monkeypatch):
    net, batch, _, shape = case(name)
    net.eval()
    view = net._view(batch) if shape.startswith("homog") else batch
    n_fwd = launches(net, lambda: net.native().forward(view, True, SEED, 1))
    lib = net.native()._lib
    finishes = []
    real = lib.hmp_mc_finish
    monkeypatch.setattr(lib, "hmp_mc_finish", lambda *a: (finishes.append(1), real(*a))[1])
    heads = 1 if shape == "room" else 2
    for T in (1, 3):
        finishes.clear()
        n_mc = launches(net, lambda: net.predict_mc(batch, samples=T, seed=SEED))
        print(name, "T", T, "mc", n_mc, "forward", n_fwd, "finish", len(finishes))
        assert n_mc == [T * (v + (1 if c == KC_LOSS else 0)) for c, v in enumerate(n_fwd)]
        assert len(finishes) == 2 * heads  # (warm + measured run) x one finishing launch per head
    with monkeypatch.context() as m:
        counter = ReadCounter(m)
        net.predict_mc(batch, samples=3, seed=SEED)
    assert counter.n == 0, counter.by  # nothing synchronises


# ---- 6. the host forms --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_predict_with_uncertainty_is_predict_mc_on_the_heads_rows(name, monkeypatch):
    net, batch, _, shape = case(name)
    net.eval()
    dev_heads = heads_of(net.predict_mc(batch, samples=5))
    host = net.predict_with_uncertainty(batch, samples=5)
    host = list(host) if isinstance(host[0], tuple) else [host]
    pred = net.predict(batch)
    pred = list(pred) if isinstance(pred, tuple) else [pred]
    assert len(host) == len(dev_heads)
    for (lab, mean, sd, ent, mi), (hl, hc, hs, he, hm), p in zip(dev_heads, host, pred):
        lab, mean, sd, ent, mi = (t.cpu() for t in (lab, mean, sd, ent, mi))
        on = lab >= 0
        assert not hl.is_cuda and hl.dtype == torch.int64 and hl.numel() == p.numel() == int(on.sum())
        assert torch.equal(hl, lab[on]) and torch.equal(hc, mean[on].gather(1, lab[on][:, None])[:, 0])
        assert torch.equal(hs, sd[on]) and torch.equal(he, ent[on]) and torch.equal(hm, mi[on])
    if name not in ("gcn", "gin"):  # one pinned buffer, one device-to-host copy
        copies = []
        real = torch.Tensor.copy_
        monkeypatch.setattr(torch.Tensor, "copy_", lambda self, src, *a, **k: (copies.append(1) if (src.is_cuda and not self.is_cuda) else None,
                                                                               real(self, src, *a, **k))[1])
        with monkeypatch.context() as m:
            counter = ReadCounter(m)
            net.predict_with_uncertainty(batch, samples=5)
        assert len(copies) == 1 and counter.n == 0, (copies, counter.by)


@pytest.mark.parametrize("name", ["hetero_gat", "hetero_htree", "homog", "homog_room", "sage_room"])
def test_evaluate_predict_mc_over_a_stream_reads_the_device_once(name, monkeypatch):
    """10 graphs in batches of 4 (a short last batch): per-graph arrays equal the per-batch calls sliced by the store's node counts"""
    if name == "sage_room":
        net, gs, _ = room_case("hetero")
        net, shape = net.to(DEV), "room"
    else:
        net, _, gs, shape = case(name)
    net.eval()
    store = GraphStore(gs, DEV)
    kw = {"label_type": "node"} if shape == "room_node" else {"label_type": "rooms"} if shape == "room" else {}
    stream = store.stream(net, 4, **kw)
    chunks = jobs.id_chunks(10, 4)
    T = 3
    evaluate.predict_mc(net, (stream, chunks), T)  # warm
    torch.cuda.synchronize()
    with monkeypatch.context() as m:
        counter = ReadCounter(m)
        got = evaluate.predict_mc(net, (stream, chunks), T)
    assert counter.n == 1, counter.by
    assert len(got) == 10
    two = shape not in ("room", "room_node")
    types = evaluate._label_types(net)
    labels = evaluate.predict(net, (stream, chunks))
    g = 0
    for ids in chunks:
        heads = heads_of(net.predict_mc(store.collate(ids), samples=T))
        offs = [np.concatenate([[0], np.cumsum(store.node_counts[t][np.asarray(ids)])]) for t in types]
        for k in range(len(ids)):
            for h, hd in enumerate(heads):
                arrays = [t.cpu().numpy()[offs[h][k]:offs[h][k + 1]] for t in hd]
                keep = arrays[0] >= 0
                mine = (got[g][h] if two else got[g])
                assert len(mine) == 5 and mine[0].dtype == np.int64 and all(a.dtype == np.float32 for a in mine[1:])
                assert all(np.array_equal(a[keep], b) for a, b in zip(arrays, mine)), (name, g, h)
                assert mine[0].shape[0] == (labels[g][h] if two else labels[g]).shape[0]
            g += 1
    per_batch = evaluate.predict_mc(net, [store.collate(ids) for ids in chunks], T)
    assert len(per_batch) == 3
    for ids, p in zip(chunks, per_batch):
        ref = heads_of(net.predict_mc(store.collate(ids), samples=T))
        for mine, hd in zip(p if two else (p,), ref):
            assert all(np.array_equal(a, b.cpu().numpy()) for a, b in zip(mine, hd))


@pytest.mark.parametrize("name", ["hetero_sage", "homog_gcn"])
def test_semisupervised_job_predict_mc(name):
    if name == "hetero_sage":
        data_type, gs, feats, params = "heterogeneous", workloads.semisupervised_graphs(12, 41), {"objects": 306, "rooms": 6}, dict(
            conv_block="GraphSAGE", hidden_dim=32, num_layers=3)
        rooms, objects = 26, 28
    else:
        data_type, gs, feats, params = "homogeneous", workloads.stanford_semisupervised_graphs(12, 42), 6, dict(
            conv_block="GCN", hidden_dim=32, num_layers=3)
        rooms, objects = 15, 35
    torch.manual_seed(4)
    job = jobs.SemiSupervisedTrainingJob(GraphDataset(data_type, gs, feats, rooms, objects), params)
    opt(job)
    job._net.to(DEV)
    labels = job.predict()
    mc = job.predict_mc(4)
    assert len(mc) == len(labels) == len(gs)
    for g, p in zip(mc, labels):
        assert isinstance(g, tuple) and len(g) == 2
        for (lab, mean, sd, ent, mi), pl, C_ in zip(g, p, (rooms, objects)):
            n = pl.shape[0]
            assert lab.dtype == np.int64 and lab.shape == (n,) and mean.shape == (n, C_) and sd.shape == ent.shape == mi.shape == (n,)
            assert ((lab >= 0) & (lab < C_)).all() and (np.abs(mean.sum(axis=1) - 1) <= 1e-5).all() if n else True
            assert (mi >= 0).all() and (mi <= ent + 1e-5).all() and (ent <= np.log(C_) + 1e-5).all()
    if name == "hetero_sage":  # the pass of the job is evaluate.predict_mc over its own stream
        stream = job._stream("all", job._dataset, torch.device(DEV), 8)
        again = evaluate.predict_mc(job._net, (stream, jobs.id_chunks(len(gs), 8)), 4)
        for g, a in zip(mc, again):
            for mine, other in zip(g, a):
                assert all(np.array_equal(x, y) for x, y in zip(mine, other))


@pytest.mark.parametrize("name", ["hetero", "gin"])
def test_room_job_predict_mc(name):
    rng = np.random.default_rng(31)
    if name == "hetero":
        data_type, gs, feats, rooms = "heterogeneous", [workloads.mp3d_like_graph(rng) for _ in range(20)], {"objects": 306, "rooms": 6}, 26
        params = dict(conv_block="GraphSAGE", hidden_dim=32, num_layers=3)
    else:
        data_type, gs, feats, rooms = "homogeneous", [workloads.stanford_like_graph(rng) for _ in range(20)], 6, 15
        params = dict(conv_block="GIN", hidden_dim=32, num_layers=3)
    dd = {"train": GraphDataset(data_type, gs[:8], feats, rooms), "val": GraphDataset(data_type, gs[8:10], feats, rooms),
          "test": GraphDataset(data_type, gs[10:], feats, rooms)}
    torch.manual_seed(3)
    job = jobs.BaseTrainingJob(dd, params)
    opt(job)
    job._net.to(DEV)
    labels = job.predict("test")
    mc = job.predict_mc("test", 4)
    assert len(mc) == len(labels) == 10
    for (lab, mean, sd, ent, mi), pl in zip(mc, labels):
        n = pl.shape[0]
        assert lab.dtype == np.int64 and lab.shape == (n,) and mean.shape == (n, rooms) and sd.shape == ent.shape == mi.shape == (n,)
        assert (mi >= 0).all() and (mi <= ent + 1e-5).all() and (ent <= np.log(rooms) + 1e-5).all() and (sd <= 0.5 + 1e-5).all()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_anything_runs():
    net, batch, _, _ = case("sage_room")
    net.eval()
    got = net.predict_mc(batch, samples=2, seed=SEED)
    n, C_ = got[1].shape
    bufs = (torch.full((n + 3,), -7, dtype=torch.int64, device=DEV), torch.full((n + 3, C_), -7.0, device=DEV),
            torch.full((n + 3,), -7.0, device=DEV), torch.full((n + 3,), -7.0, device=DEV), torch.full((n + 3,), -7.0, device=DEV))
    views = net.predict_mc(batch, samples=2, seed=SEED, out=bufs)
    assert all(v.data_ptr() == b.data_ptr() and torch.equal(v, g) and bool((b[n:] == -7).all()) for v, b, g in zip(views, bufs, got))
    for bad in (bufs[:4], bufs[0], (bufs[0][:n - 1],) + bufs[1:], (bufs[0], bufs[1][:, :C_ - 1].contiguous()) + bufs[2:],
                tuple(b.cpu() for b in bufs), (bufs[0].int(),) + bufs[1:]):
        with pytest.raises(_lib.HydraMPError, match="out"):
            net.predict_mc(batch, samples=2, out=bad)
    for samples in (0, 4097):
        with pytest.raises(_lib.HydraMPError, match="samples must be"):
            net.predict_mc(batch, samples=samples)
    with pytest.raises(_lib.HydraMPError, match="first_step must be"):
        net.predict_mc(batch, samples=2, first_step=2 ** 32 - 1)
    last = heads_of(net.predict_mc(batch, samples=1, seed=SEED, first_step=2 ** 32 - 1))  # the last step of the 32-bit counter
    assert bool((last[0][0] >= 0).all())
    two, b2, _, _ = case("hetero_gat")
    with pytest.raises(_lib.HydraMPError, match="no members"):
        two.native().predict_mc(b2, 2, SEED, members=torch.ones(3, dtype=torch.bool, device=DEV))
    lin, b3, _, _ = case("homog")
    with pytest.raises(_lib.HydraMPError, match="members"):
        lin.native().predict_mc(lin._view(b3), 2, SEED)
