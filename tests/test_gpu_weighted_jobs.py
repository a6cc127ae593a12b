"""optimization_params["class_weight"] in the training jobs, and balanced accuracy.

1. BaseTrainingJob.train with class_weight="balanced" equals, bit for bit, the hand-written loop of tests/test_gpu_training_job.py
   over train_step(class_weight=store.class_weights(...)): the same kernels in the same order, and the epoch's loss is the
   weight-normalised mean (the steps' weighted sums over the steps' sums of weights) formed with the same products and sums.
2. The same for SemiSupervisedTrainingJob with a per-head dict, the weights from the rows of train_mask.
3. A GCN job on the op path: every step's loss is net.loss(..., weight=w), bit-equal between job and hand loop, and equal to
   torch.nn.functional.cross_entropy(weight=w) on the same logits within the tolerance of tests/test_gpu_ops.py (1e-5).
4. evaluate.accuracy(balanced=True) is the mean per-class recall of the confusion matrix it returns.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import test_gpu_training_job as tj  # noqa: E402  (datasets, the hand loop and the bit comparison of the unweighted jobs)
from hydra_gnn_amd import _lib, evaluate, jobs  # noqa: E402
from hydra_gnn_amd.store import GraphStore  # noqa: E402

DEV = tj.DEV
B, LR, WD = tj.B, tj.LR, tj.WD
EPOCHS = 3
KW = dict(tj.TRAIN_KW, min_log_epoch=0)  # three epochs: every one of them may be the best


def step_pair(step):
    """(loss, weight) of the last step as the epoch record accumulates them: loss_sum / weight_sum in double, weight = weight_sum"""
    t = step.grads[step.net.n_active: step.net.n_active + 2].tolist()
    return t[0] / (t[1] if t[1] > 0.0 else 1.0), t[1]


def test_room_job_with_balanced_weights_equals_the_hand_loop(tmp_path):
    name = "hetero_sage"
    job = tj.make_room_job(name)
    net = job._net.to(DEV)
    split = {s: job.get_dataset(s).graphs for s in ("train", "val", "test")}
    stores = {s: GraphStore(g, DEV) for s, g in split.items()}
    streams = {s: stores[s].stream(net, B, "rooms") for s in stores}
    w = stores["train"].class_weights("rooms", n_classes=26, ignored_label=25)
    assert w.shape == (26,) and float(w[25]) == 0.0 and float(w.max()) > 1.0  # the ignored class has no support; rare classes weigh more
    step = net.train_step(lr=LR, weight_decay=WD, ignored_label=25, use_graph=False, class_weight=w)

    def train_batch(ids):
        step.run(streams["train"].next(ids))
        return step_pair(step)

    acc = lambda s: evaluate.accuracy(net, (streams[s], tj.chunks(len(split[s]))))  # noqa: E731
    torch.manual_seed(17)
    hand = tj.HandLoop(net, len(split["train"]), step.set_lr).run(EPOCHS, train_batch, lambda: acc("val"), min_log_epoch=0)
    net.eval()
    hand["test_result"] = acc("test")
    hand["state"] = {k: v.clone() for k, v in net.state_dict().items()}

    job = tj.make_room_job(name)
    torch.manual_seed(17)
    out = job.train(str(tmp_path), dict(tj.OPT, num_epochs=EPOCHS, class_weight="balanced"), **KW)
    tj.check_equal(out, hand)
    # the weights changed the run: the unweighted job's losses are others
    job0 = tj.make_room_job(name)
    torch.manual_seed(17)
    out0 = job0.train(str(tmp_path), dict(tj.OPT, num_epochs=EPOCHS), **KW)
    assert tj.bits(out0[2]["loss"]) != tj.bits(out[2]["loss"])
    # explicit weights take the same road
    job1 = tj.make_room_job(name)
    torch.manual_seed(17)
    out1 = job1.train(str(tmp_path), dict(tj.OPT, num_epochs=EPOCHS, class_weight=w.cpu().tolist()), **KW)
    assert tj.bits(out1[2]["loss"]) == tj.bits(out[2]["loss"])
    with pytest.raises(_lib.HydraMPError, match="unknown scheme 'inverse'"):
        tj.make_room_job(name).train(str(tmp_path), dict(tj.OPT, num_epochs=1, class_weight="inverse"), **KW)
    with pytest.raises(_lib.HydraMPError, match="wrong length"):
        tj.make_room_job(name).train(str(tmp_path), dict(tj.OPT, num_epochs=1, class_weight=[1.0] * 5), **KW)


@pytest.mark.parametrize("name", ["hetero_sage", "homog_sage"])
def test_semisupervised_job_with_a_per_head_dict_equals_the_hand_loop(name, tmp_path):
    job = tj.make_semi_job(name)
    net = job._net.to(DEV)
    gs = job.get_dataset().graphs
    store = GraphStore(gs, DEV)
    stream = store.stream(net, B)
    classes = net.native().head_classes()
    w_rooms = store.class_weights("rooms", mask="train_mask", n_classes=classes[0], ignored_label=-100)
    w_objects = [0.5 + (c % 3) for c in range(classes[1])]  # explicit weights for the second head
    step = net.semisupervised_step(lr=LR, weight_decay=WD, use_graph=False, class_weight={"rooms": w_rooms, "objects": w_objects})

    def train_batch(ids):
        step.run(stream.next(ids), mask="train_mask")
        return step.loss(), len(ids)  # loss.item() * batch.num_graphs

    acc = lambda m: evaluate.semisupervised_accuracy(net, (stream, tj.chunks(len(gs))), m)  # noqa: E731
    torch.manual_seed(18)
    hand = tj.HandLoop(net, len(gs), step.set_lr, loss_div=len(gs)).run(EPOCHS, train_batch, lambda: acc("val_mask"), min_log_epoch=0)
    net.eval()
    hand["test_result"] = acc("test_mask")
    hand["state"] = {k: v.clone() for k, v in net.state_dict().items()}

    job = tj.make_semi_job(name)
    torch.manual_seed(18)
    cw = {"rooms": "balanced", "objects": w_objects}
    out = job.train(str(tmp_path), dict(tj.OPT, num_epochs=EPOCHS, class_weight=cw), **KW)
    tj.check_equal(out, hand)


def test_gcn_job_on_the_op_path(tmp_path):
    data_type, gs, feats, rooms, _ = tj.room_case("gin")
    params = dict(conv_block="GCN", hidden_dim=32, num_layers=3)

    def make():
        dd = {"train": tj.GraphDataset(data_type, gs[:48], feats, rooms), "val": tj.GraphDataset(data_type, gs[48:64], feats, rooms),
              "test": tj.GraphDataset(data_type, gs[64:], feats, rooms)}
        torch.manual_seed(3)
        return jobs.BaseTrainingJob(dd, params)

    job = make()
    net = job._net.to(DEV)
    split = {s: job.get_dataset(s).graphs for s in ("train", "val", "test")}
    stores = {s: GraphStore(g, DEV) for s, g in split.items()}
    w = stores["train"].class_weights("rooms", n_classes=rooms, ignored_label=25)
    assert int((w > 0).sum()) == 3  # (the dataset's rooms carry three of the 15 classes)
    opt = torch.optim.Adam(net.parameters(), lr=LR, weight_decay=WD)
    checked = []

    def train_batch(ids):  # the reference's body with the weighted loss
        b = stores["train"].collate(ids)
        opt.zero_grad()
        pred = net(b)
        label = b.y[b.room_mask]
        mask = label != 25
        loss = net.loss(pred, label, mask, weight=w)
        loss.backward()
        opt.step()
        # F.cross_entropy(weight=) semantics on the same logits
        ref = F.cross_entropy(pred.detach().double().cpu()[mask.cpu()], label[mask].cpu(), weight=w.double().cpu())
        torch.testing.assert_close(loss.detach().double().cpu(), ref, atol=1e-5, rtol=1e-5)
        checked.append(float(ref))
        ws = float(w.double()[label[mask]].sum())
        return float(loss.detach()), ws

    def set_lr(v):
        for g in opt.param_groups:
            g["lr"] = v

    acc = lambda s: evaluate.accuracy(net, [stores[s].collate(ids) for ids in tj.chunks(len(split[s]))])  # noqa: E731
    torch.manual_seed(17)
    hand = tj.HandLoop(net, len(split["train"]), set_lr).run(EPOCHS, train_batch, lambda: acc("val"), min_log_epoch=0)
    net.eval()
    hand["test_result"] = acc("test")
    hand["state"] = {k: v.clone() for k, v in net.state_dict().items()}
    assert len(checked) == EPOCHS * 3

    job = make()
    torch.manual_seed(17)
    net2, (max_val_acc, test_result), info = job.train(str(tmp_path), dict(tj.OPT, num_epochs=EPOCHS, class_weight="balanced"), **KW)
    # the same steps: validation results, best epoch and the final state are the hand loop's, bit for bit
    assert info["validation_result"] == hand["vals"] and info["best_epoch"] == hand["best_epoch"] and max_val_acc == hand["max_val_acc"]
    state = net2.state_dict()
    for k, v in hand["state"].items():
        assert torch.equal(state[k], v), k
    assert test_result == hand["test_result"]
    # the epoch's loss is the weight-normalised mean; the device record forms loss * ws in float32 before the double sums, so it
    # agrees with the hand loop's double arithmetic to float32 rounding
    np.testing.assert_allclose(info["loss"], hand["losses"], rtol=1e-6)


def test_balanced_accuracy_is_the_mean_recall_of_the_confusion_matrix():
    job = tj.make_room_job("hetero_sage")
    job._net.to(DEV)
    acc, matrix, bal = job.test("test", get_per_label_accuracy=True, get_balanced_accuracy=True)
    assert acc == job.test("test") and (acc, bal) == job.test("test", get_balanced_accuracy=True)
    assert matrix.shape == (25, 26)
    support = matrix.sum(axis=1)
    have = support > 0
    assert have.sum() > 0  # (classes without support do not enter the mean)
    want = float(np.mean(np.diag(matrix[:, :25])[have] / support[have]))
    assert bal == want
    assert acc == float(np.diag(matrix[:, :25]).sum() / support.sum())
