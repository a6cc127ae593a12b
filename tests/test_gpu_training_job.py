"""GPU checks of hydra_gnn_amd.jobs and csrc/epoch.hip.

1. A job's ``train()`` equals the hand-written loop of the reference's shape (``step.loss()`` per step into a Python double, an
   accuracy read per epoch, ``deepcopy(state_dict())`` on strict improvement, ``load_state_dict``) EXACTLY: both run the same
   kernels in the same order, and the device record forms the loss sum with the same rounded products and sums.
2. ``hmp_epoch_close`` alone on synthetic counter sequences and a segment table whose contents change every epoch, at several
   grid sizes.
3. Early stopping ends at the hand loop's epoch.
4. The number of device-to-host reads of ``train()``.
"""
import copy
import ctypes as C
import struct

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

pytestmark = pytest.mark.gpu

from hydra_gnn_amd import _lib, evaluate, jobs, workloads  # noqa: E402
from hydra_gnn_amd.data import heterogeneous_htree_to_homogeneous  # noqa: E402
from hydra_gnn_amd.store import GraphStore  # noqa: E402

DEV = "cuda:0"
B = 16
LR, WD = 0.004, 0.001
HT_DIMS = {"object": 306, "room": 6, "object-room": 6, "room-room": 6, "object_virtual": 306, "room_virtual": 6}
GAT3 = dict(GAT_hidden_dims=[16, 16], GAT_heads=[2, 2, 2], GAT_concats=[True, True, False])
TRAIN_KW = dict(decay_epochs=2, decay_rate=0.5, min_log_epoch=1)


# ---- a dataset as the jobs read one ---------------------------------------------------------------------------------------
class _Info:
    def __init__(self, features, rooms, objects):
        self._f, self._r, self._o = features, rooms, objects

    def num_node_features(self):
        return self._f

    def num_room_labels(self):
        return self._r

    def num_object_labels(self):
        return self._o


class GraphDataset:
    def __init__(self, data_type, graphs, features, rooms, objects=None):
        self._type, self.graphs, self._info = data_type, list(graphs), _Info(features, rooms, objects)

    def data_type(self):
        return self._type

    def __len__(self):
        return len(self.graphs)

    def __getitem__(self, i):
        return self.graphs[i]

    def get_data(self, i):
        return self._info


def _htree_graphs(n, seed):
    npz = np.load(workloads.HTREE_FIXTURE)
    rng = np.random.Generator(np.random.PCG64(seed))
    k = int(npz["n_graphs"])
    return [workloads.htree_graph(npz, i % k, rng) for i in range(n)]


def _homog_htree_graphs(n, seed):
    out = []
    for g in _htree_graphs(n, seed):
        d = heterogeneous_htree_to_homogeneous(g)
        del d.__dict__["edge_type"]
        out.append(d)
    return out


def _stanford_room_graphs(rng, n):
    """Stanford-like graphs (ONE room each) whose room label is a function of the room's size feature, three of the 15 classes: with
    the generator's random labels the 16 validation rooms would often all be wrong, and a run without any improvement has no best
    state (the reference fails there too)"""
    gs = [workloads.stanford_like_graph(rng) for _ in range(n)]
    for g in gs:
        g.y[0] = min(int((float(g.x[0, 3]) - 0.1) / 2.9 * 3), 2)
    return gs


def room_case(name):
    """(data_type, 80 graphs, node features, room classes, network params)"""
    rng = np.random.default_rng(31)
    if name == "hetero_sage":
        gs = [workloads.mp3d_like_graph(rng) for _ in range(80)]
        return "heterogeneous", gs, {"objects": 306, "rooms": 6}, 26, dict(conv_block="GraphSAGE", hidden_dim=32, num_layers=3)
    if name == "hetero_htree_sage":
        return ("heterogeneous_htree", _htree_graphs(80, 32), dict(HT_DIMS), 26,
                dict(conv_block="GraphSAGE", hidden_dim=32, num_layers=3, disable_initialization=True))
    if name == "homog_sage":
        return "homogeneous", _stanford_room_graphs(rng, 80), 6, 15, dict(conv_block="GraphSAGE", hidden_dim=32, num_layers=3)
    if name == "homog_htree_gat":
        return "homogeneous_htree", _homog_htree_graphs(80, 33), 306, 26, dict(conv_block="GAT", disable_initialization=True, **GAT3)
    assert name == "gin"
    return "homogeneous", _stanford_room_graphs(rng, 80), 6, 15, dict(conv_block="GIN", hidden_dim=32, num_layers=3)


def make_room_job(name, seed=3):
    data_type, gs, feats, rooms, params = room_case(name)
    dd = {"train": GraphDataset(data_type, gs[:48], feats, rooms), "val": GraphDataset(data_type, gs[48:64], feats, rooms),
          "test": GraphDataset(data_type, gs[64:], feats, rooms)}
    torch.manual_seed(seed)
    return jobs.BaseTrainingJob(dd, params)


def semi_case(name):
    if name == "hetero_sage":
        return ("heterogeneous", workloads.semisupervised_graphs(48, 41), {"objects": 306, "rooms": 6}, 26, 28,
                dict(conv_block="GraphSAGE", hidden_dim=32, num_layers=3))
    if name == "homog_sage":
        return ("homogeneous", workloads.stanford_semisupervised_graphs(48, 42), 6, 15, 35,
                dict(conv_block="GraphSAGE", hidden_dim=32, num_layers=3))
    assert name == "hetero_htree_gat"
    return ("heterogeneous_htree", workloads.semisupervised_htree_graphs(48, 43), dict(HT_DIMS), 15, 35,
            dict(conv_block="GAT", disable_initialization=True, **GAT3))


def make_semi_job(name, seed=4):
    data_type, gs, feats, rooms, objects, params = semi_case(name)
    torch.manual_seed(seed)
    return jobs.SemiSupervisedTrainingJob(GraphDataset(data_type, gs, feats, rooms, objects), params)


# ---- the hand loops: today's public pieces, the reference's bookkeeping on the host ------------------------------------------
def chunks(n):
    return [list(range(i, min(i + B, n))) for i in range(0, n, B)]


class HandLoop:
    """BaseTrainingJob.train's bookkeeping (base_training_job.py:191-253) around a ``train_batch(ids) -> (loss, weight)`` and a
    ``val() -> accuracy``"""

    def __init__(self, net, n_train, set_lr, loss_div=None):
        self.net, self.n_train, self.set_lr, self.loss_div = net, n_train, set_lr, loss_div

    def run(self, num_epochs, train_batch, val, early_stop_window=-1, decay_epochs=2, decay_rate=0.5, min_log_epoch=1):
        net = self.net
        loader = DataLoader(range(self.n_train), batch_size=B, shuffle=True)
        max_val_acc, best, best_epoch, early_stop_step = 0, None, -1, 0
        losses, vals = [], []
        for epoch in range(num_epochs):
            early_stop_step += 1
            self.set_lr(LR * decay_rate ** (epoch // decay_epochs))
            total_loss, weights = 0.0, 0
            net.train()
            for ids in loader:
                loss, w = train_batch(ids.tolist())
                total_loss += loss * w
                weights += w
            total_loss /= self.loss_div if self.loss_div is not None else weights
            losses.append(total_loss)
            net.eval()
            val_result = val()
            vals.append(val_result)
            if epoch >= min_log_epoch and val_result > max_val_acc:
                max_val_acc, best, best_epoch, early_stop_step = val_result, copy.deepcopy(net.state_dict()), epoch, 0
            if early_stop_step == early_stop_window and epoch > early_stop_window:
                break
        net.load_state_dict(best)
        return dict(losses=losses, vals=vals, max_val_acc=max_val_acc, best_epoch=best_epoch, num_epochs=epoch + 1)


def hand_room(name, num_epochs, seed, **kw):
    job = make_room_job(name)  # same seed, same construction: the same initial weights and dropout seed
    net = job._net.to(DEV)
    ignored = 25
    split = {s: job.get_dataset(s).graphs for s in ("train", "val", "test")}
    stores = {s: GraphStore(g, DEV) for s, g in split.items()}
    hetero = not name.startswith("homog") and name != "gin"
    if hetero:
        label_type = "room_virtual" if "htree" in name else "rooms"
        streams = {s: stores[s].stream(net, B, label_type) for s in stores}
        step = net.train_step(lr=LR, weight_decay=WD, ignored_label=ignored, use_graph=False)

        def train_batch(ids):
            step.run(streams["train"].next(ids))
            return step.loss(), int(sum((split["train"][i][label_type].y != ignored).sum() for i in ids))

        acc = lambda s: evaluate.accuracy(net, (streams[s], chunks(len(split[s]))))
        set_lr = step.set_lr
    elif name != "gin":
        step = net.train_step(lr=LR, weight_decay=WD, ignored_label=ignored, use_graph=False)

        def train_batch(ids):
            b = stores["train"].collate(ids)
            labels = torch.where(b.room_mask, b.y, torch.full_like(b.y, ignored))
            step(b, labels)
            return step.loss(), int((labels != ignored).sum().item())

        acc = lambda s: evaluate.accuracy(net, [stores[s].collate(ids) for ids in chunks(len(split[s]))])
        set_lr = step.set_lr
    else:
        opt = torch.optim.Adam(net.parameters(), lr=LR, weight_decay=WD)

        def train_batch(ids):  # base_training_job.py:202-219
            b = stores["train"].collate(ids)
            opt.zero_grad()
            pred = net(b)
            label = b.y[b.room_mask]
            mask = label != ignored
            loss = net.loss(pred, label, mask)
            loss.backward()
            opt.step()
            return loss.item(), mask.sum().item()

        def set_lr(v):
            for g in opt.param_groups:
                g["lr"] = v

        acc = lambda s: evaluate.accuracy(net, [stores[s].collate(ids) for ids in chunks(len(split[s]))])
    torch.manual_seed(seed)
    out = HandLoop(net, len(split["train"]), set_lr).run(num_epochs, train_batch, lambda: acc("val"), **kw)
    net.eval()
    out["test_result"] = acc("test")
    out["state"] = {k: v.clone() for k, v in net.state_dict().items()}
    return out


def hand_semi(name, num_epochs, seed, **kw):
    job = make_semi_job(name)
    net = job._net.to(DEV)
    gs = job.get_dataset().graphs
    stream = GraphStore(gs, DEV).stream(net, B)
    step = net.semisupervised_step(lr=LR, weight_decay=WD, use_graph=False)

    def train_batch(ids):
        step.run(stream.next(ids), mask="train_mask")
        return step.loss(), len(ids)  # loss.item() * batch.num_graphs

    acc = lambda m: evaluate.semisupervised_accuracy(net, (stream, chunks(len(gs))), m)
    torch.manual_seed(seed)
    out = HandLoop(net, len(gs), step.set_lr, loss_div=len(gs)).run(num_epochs, train_batch, lambda: acc("val_mask"), **kw)
    net.eval()
    out["test_result"] = acc("test_mask")
    out["state"] = {k: v.clone() for k, v in net.state_dict().items()}
    return out


def bits(values):
    return [struct.pack("<d", float(v)).hex() for v in values]


def check_equal(job_out, hand):
    net, (max_val_acc, test_result), info = job_out
    print("job  losses", info["loss"], "vals", info["validation_result"], "best", info["best_epoch"], max_val_acc, test_result)
    print("hand losses", hand["losses"], "vals", hand["vals"], "best", hand["best_epoch"], hand["max_val_acc"], hand["test_result"])
    assert info["num_epochs"] == hand["num_epochs"]
    assert bits(info["loss"]) == bits(hand["losses"]), "per-epoch losses are not bit-equal"
    assert info["validation_result"] == hand["vals"]
    assert info["best_epoch"] == hand["best_epoch"] and max_val_acc == hand["max_val_acc"]
    state = net.state_dict()
    assert list(state) == list(hand["state"])
    for k, v in hand["state"].items():
        assert state[k].dtype == v.dtype and torch.equal(state[k], v), k
    assert test_result == hand["test_result"]


OPT = {"lr": LR, "weight_decay": WD, "batch_size": B, "shuffle": True}


# ---- 1. job == hand loop ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hetero_sage", "hetero_htree_sage", "homog_sage", "homog_htree_gat", "gin"])
def test_room_job_equals_the_hand_loop(name, tmp_path):
    hand = hand_room(name, 6, seed=17)
    job = make_room_job(name)
    torch.manual_seed(17)
    out = job.train(str(tmp_path), dict(OPT, num_epochs=6), **TRAIN_KW)
    check_equal(out, hand)
    if name == "gin":
        assert any(k.endswith("num_batches_tracked") for k in hand["state"])
    assert job.test("test") == hand["test_result"]


@pytest.mark.parametrize("name", ["hetero_sage", "homog_sage", "hetero_htree_gat"])
def test_semisupervised_job_equals_the_hand_loop(name, tmp_path):
    hand = hand_semi(name, 6, seed=18)
    job = make_semi_job(name)
    torch.manual_seed(18)
    out = job.train(str(tmp_path), dict(OPT, num_epochs=6), **TRAIN_KW)
    check_equal(out, hand)
    assert job.test(mask_name="test_mask") == hand["test_result"]


# ---- 2. hmp_epoch_close alone -----------------------------------------------------------------------------------------------
def _fill(tensors, epoch):
    """contents that differ between epochs and between positions"""
    for k, t in enumerate(tensors):
        n = t.numel()
        v = (torch.arange(n, dtype=torch.int64) * (2 * k + 3) + 1000 * (epoch + 1) + k) % 251
        t.copy_(v.to(t.dtype).view(t.shape))


@pytest.mark.parametrize("grid_blocks", [None, 1, 3, 64, 5000])
def test_epoch_close_keeps_the_snapshot_of_strict_improvements(grid_blocks):
    dev = torch.device(DEV)
    raw = torch.zeros(4200, dtype=torch.uint8, device=dev)
    tensors = [torch.zeros(1, dtype=torch.float32, device=dev),      # 4 B
               torch.zeros((), dtype=torch.int64, device=dev),       # BatchNorm's num_batches_tracked
               raw[1:4100],                                          # 4099 B at an odd address
               torch.zeros(300_001, dtype=torch.float32, device=dev),  # above one workgroup's worth, not a multiple of 16 B
               torch.zeros(7, dtype=torch.uint8, device=dev)]
    book = jobs.EpochBook(dev, 8, tensors, grid_blocks=grid_blocks)
    initial = [t.clone() for t in tensors]
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    seq = [(3, 10), (3, 10), (5, 10), (4, 10), (0, 0), (5, 10), (6, 10)]
    min_log_epoch, window = 1, 2
    # the reference's bookkeeping on the host
    max_acc, ess, want_snapshot, want_rows, stop_at, best_epoch = 0, 0, initial, [], None, 0
    losses = torch.tensor([1.25, 0.3333333, 2.7182817], dtype=torch.float32)
    loss_dev = losses.to(dev)
    cnt_dev = torch.tensor([7.0, 0.0, 12.0], dtype=torch.float32, device=dev)
    for epoch, (c, t) in enumerate(seq):
        _fill(tensors, epoch)
        acc_loss, acc_w = 0.0, 0.0
        for i in range(3):  # loss_sum / max(count, 1), weight = count
            book.accumulate(loss_dev[i:], cnt_dev[i:])
            cnt = float(cnt_dev[i])
            acc_loss += (float(losses[i]) / max(cnt, 1.0)) * cnt
            acc_w += cnt
        w64 = torch.tensor(3, dtype=torch.int64, device=dev)
        book.accumulate(loss_dev[2:], None, w64)  # a loss scalar with a device int64 weight
        acc_loss += float(losses[2]) * 3.0
        acc_w += 3.0
        book.accumulate(loss_dev[0:], None, None, 16.0)  # ... and with a host weight
        acc_loss += float(losses[0]) * 16.0
        acc_w += 16.0
        counts.copy_(torch.tensor([c, t]))
        book.close(counts, 0.0, min_log_epoch, window)
        ess += 1
        improved = t > 0 and epoch >= min_log_epoch and c / t > max_acc
        if improved:
            max_acc, ess, best_epoch = c / t, 0, epoch
            want_snapshot = [x.clone() for x in tensors]
        if ess == window and epoch > window and stop_at is None:
            stop_at = epoch
        want_rows.append((acc_loss / acc_w, c / t if t else 0.0, c, t, int(improved)))
        assert counts.cpu().tolist() == [0, 0]
        for k, (got, want) in enumerate(zip(book.snapshot, want_snapshot)):
            assert torch.equal(got, want), (epoch, k)
        assert bool(book.status() & _lib.EPOCH_STOP) == (stop_at is not None), epoch
        assert bool(book.status() & _lib.EPOCH_EMPTY_VAL) == (epoch >= 4), epoch
    assert int(raw[0]) == 0 and int(raw[4100:].sum()) == 0
    ctl, rows = book.read()
    assert (ctl.epoch, ctl.best_epoch, ctl.early_stop_step, ctl.max_val_acc) == (len(seq), best_epoch, ess, max_acc)
    assert ctl.loss_acc == 0.0 and ctl.weight_acc == 0.0
    assert stop_at == 4 and best_epoch == 6  # 1: first kept, 2: improves, 3: no, 4: 0/0, 5: tie (kept out), 6: improves
    got_rows = [(r.loss, r.val_acc, r.correct, r.total, r.improved) for r in rows]
    assert bits([r[0] for r in got_rows]) == bits([r[0] for r in want_rows])
    assert [r[1:] for r in got_rows] == [r[1:] for r in want_rows]
    # restore: the snapshot back over a state that moved on
    _fill(tensors, 99)
    book.restore()
    for k, (got, want) in enumerate(zip(tensors, want_snapshot)):
        assert torch.equal(got, want), k
    assert int(raw[0]) == 0 and int(raw[4100:].sum()) == 0


def test_epoch_close_sums_both_heads_and_divides_by_the_dataset():
    dev = torch.device(DEV)
    state = torch.arange(10, dtype=torch.float32, device=dev)
    book = jobs.EpochBook(dev, 2, [state])
    loss = torch.tensor([0.75], dtype=torch.float32, device=dev)
    book.accumulate(loss, None, None, 16.0)
    book.accumulate(loss, None, None, 5.0)
    counts = torch.tensor([1, 4, 2, 6], dtype=torch.int64, device=dev)
    book.close(counts, 21.0, 0, -1)
    state += 1
    counts.copy_(torch.tensor([1, 4, 2, 6]))
    book.close(counts, 21.0, 0, -1)  # a tie: the first snapshot stays
    counts.copy_(torch.tensor([1, 4, 2, 6]))  # every close zeroes the counters: an unfilled pass would be 0 / 0 (the empty-pass bit)
    book.close(counts, 21.0, 0, -1)  # beyond the log's capacity: no row is written
    ctl, rows = book.read()
    assert ctl.epoch == 3 and len(rows) == 2 and ctl.max_val_acc == 3 / 10 and ctl.best_epoch == 0 and ctl.status == 0
    assert rows[0].loss == (0.75 * 16.0 + 0.75 * 5.0) / 21.0 and (rows[0].correct, rows[0].total, rows[0].improved) == (3, 10, 1)
    assert rows[1].improved == 0 and rows[1].loss == 0.0
    assert torch.equal(book.snapshot[0], torch.arange(10, dtype=torch.float32, device=dev))
    with pytest.raises(_lib.HydraMPError):
        book.close(torch.zeros(3, dtype=torch.int64, device=dev))
    with pytest.raises(_lib.HydraMPError):
        jobs.EpochBook(dev, 2, [torch.zeros(1, device=dev)] * 65)


# ---- 3. early stopping ------------------------------------------------------------------------------------------------------
def test_early_stopping_ends_at_the_hand_loops_epoch(tmp_path):
    hand = hand_room("hetero_sage", 14, seed=19, early_stop_window=2)
    job = make_room_job("hetero_sage")
    torch.manual_seed(19)
    out = job.train(str(tmp_path), dict(OPT, num_epochs=14), early_stop_window=2, **TRAIN_KW)
    check_equal(out, hand)
    print("stopped after", out[2]["num_epochs"], "of 14 epochs")


# ---- 4. host reads ----------------------------------------------------------------------------------------------------------
class ReadCounter:
    """counts device-to-host reads: Tensor.item / cpu / tolist / numpy on a device tensor and the library's synchronising entries"""

    TENSOR = ("item", "cpu", "tolist", "numpy")
    ENTRIES = ("hmp_epoch_read", "hmp_epoch_read_status", "hmp_net_read_state", "hmp_timer_elapsed_ms")

    def __init__(self, monkeypatch):
        self.n = 0
        self.by = {}
        lib = _lib.load()
        for name in self.TENSOR:
            monkeypatch.setattr(torch.Tensor, name, self._tensor(name, getattr(torch.Tensor, name)))
        for name in self.ENTRIES:
            monkeypatch.setattr(lib, name, self._entry(name, getattr(lib, name)))

    def _hit(self, name):
        self.n += 1
        self.by[name] = self.by.get(name, 0) + 1

    def _tensor(self, name, orig):
        def wrapped(t, *a, **k):
            if t.is_cuda:
                self._hit(name)
            return orig(t, *a, **k)

        return wrapped

    def _entry(self, name, orig):
        def wrapped(*a):
            self._hit(name)
            return orig(*a)

        return wrapped


@pytest.mark.parametrize("kind,name", [("room", "hetero_sage"), ("semi", "hetero_sage"), ("semi", "homog_sage")])
def test_train_reads_the_device_twice_whatever_the_epoch_count(kind, name, tmp_path, monkeypatch):
    seen = []
    for num_epochs in (2, 5):
        job = make_room_job(name) if kind == "room" else make_semi_job(name)
        torch.manual_seed(20)
        with monkeypatch.context() as m:
            counter = ReadCounter(m)
            _, _, info = job.train(str(tmp_path), dict(OPT, num_epochs=num_epochs), **TRAIN_KW)
        print(kind, name, num_epochs, "epochs:", counter.by)
        assert info["num_epochs"] == num_epochs
        assert counter.n <= 2, counter.by
        seen.append(counter.n)
    assert seen[0] == seen[1]


def test_train_with_early_stopping_reads_one_status_word_per_epoch(tmp_path, monkeypatch):
    job = make_room_job("hetero_sage")
    torch.manual_seed(21)
    with monkeypatch.context() as m:
        counter = ReadCounter(m)
        _, _, info = job.train(str(tmp_path), dict(OPT, num_epochs=6), early_stop_window=4, **TRAIN_KW)
    print("early stopping:", counter.by, info["num_epochs"], "epochs")
    assert counter.n <= info["num_epochs"] + 2, counter.by
    assert counter.by.get("hmp_epoch_read_status", 0) == info["num_epochs"]
