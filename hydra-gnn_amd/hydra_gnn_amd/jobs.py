"""``BaseTrainingJob`` / ``SemiSupervisedTrainingJob`` -- the reference's training jobs (``src/hydra_gnn/base_training_job.py``,
``semisupervised_training_job.py``) with the epoch loop's bookkeeping on the device.

The reference's ``train()`` reads the loss after every step (``loss.item() * mask.sum().item()``, :218), the validation count after
every epoch and deep-copies ``state_dict()`` on every improvement.  Here

* every split is uploaded once (:class:`store.GraphStore`) and served by one :class:`store.BatchStream`;
* the loop body is the fused step on device-collated batches (``train_step(...).run(stream.next(ids))`` /
  ``semisupervised_step(...).run(..., mask="train_mask")``);
* the weighted loss sum, the best validation accuracy, the best-state snapshot and the early-stop counter live in one device
  record (:class:`EpochBook`: ``hmp_epoch_accumulate`` after a step, ``hmp_epoch_close`` after the validation pass,
  ``hmp_epoch_restore`` after the loop), read ONCE after the loop (``hmp_epoch_read``).

Host reads per ``train()``: one after the loop plus the test pass's one; with ``early_stop_window != -1`` one 4-byte status read
per epoch on top.  ``verbose=True`` adds the reads its printing needs (a training-accuracy pass per epoch, a record read every ten
epochs).  The executor's sticky input-data status word is not read inside ``train()``; ``net.native().check_status()`` reads it.

Homogeneous room classifiers stream like the others: their stream writes the labels outside ``room_mask`` as ``ignored_label`` in
the collation launch and carries ``room_mask`` as the row filter of the counts.  GCN / GIN, which the fused step does not cover,
keep a loop body of their own on ``store.collate`` batches with the same bookkeeping: the reference's body (``net(batch)``,
``net.loss``, ``backward``, ``torch.optim.Adam``; their forward compacts rows with boolean masks and therefore synchronises inside
torch).

Shuffling.  Epoch ``e``'s training order is what ``torch.utils.data.DataLoader(range(n), batch_size, shuffle=True)`` yields in its
``e``-th iteration, and that loader is the only consumer of torch's global generator inside ``train()``.  The validation and test
passes are never shuffled: their integer counts do not depend on the order.  The reference passes ``shuffle`` to those loaders
too and so draws extra seeds from the global generator every epoch -- a run here and a run of the reference under the same
``torch.manual_seed`` see different training permutations from the second epoch on.

Class weights.  ``optimization_params["class_weight"]``: None (the default: the unweighted loss), ``"balanced"`` or explicit
weights (a tensor or a sequence with one entry per class); the semi-supervised job also takes a dict per head,
``{"rooms": ..., "objects": ...}``.  ``"balanced"`` is computed on the device from the training split's resident store
(``GraphStore.class_weights``; the semi-supervised job: the rows of ``train_mask``) at the start of ``train()``, after the node
split of that run.  The weights reach the fused step (``train_step(class_weight=...)``) and the GCN / GIN body
(``net.loss(..., weight=...)``) alike.  The loss is then ``sum(w[y] * nll) / sum(w[y])``, and the epoch's logged loss of the
room job is that weight-normalised mean over the epoch (the steps' weighted sums over the steps' sums of weights); the
semi-supervised job keeps ``sum(batch loss * num_graphs) / len(dataset)`` with the batch loss weight-normalised.  Validation and
test accuracies do not depend on the weights; ``test(..., get_balanced_accuracy=True)`` adds the mean per-class recall.

Scalars go to ``tensorboardX.SummaryWriter(log_folder)`` when that module is installed, else to ``log_folder/scalars.json``
(``{"loss": [...], "validation result": [...]}``); both are written after the loop from the device log.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys
import time
from typing import Iterable, List, Optional, Sequence, Tuple

import torch

from . import _lib, evaluate
from .models import (HeterogeneousNetwork, HeterogeneousNeuralTreeNetwork, HomogeneousNetwork,
                     HomogeneousNeuralTreeNetwork)


def id_chunks(n: int, batch_size: int) -> List[List[int]]:
    """graph ids 0..n-1 in order, cut into batches (the unshuffled passes)"""
    return [list(range(i, min(i + batch_size, n))) for i in range(0, n, batch_size)]


def order_loader(n: int, batch_size: int, shuffle: bool = True):
    """The index loader whose iterations are the epochs' training orders: each ``iter()`` draws from torch's global generator
    exactly what a ``DataLoader`` over the dataset itself draws, and yields lists of graph ids."""
    from torch.utils.data import DataLoader

    return DataLoader(range(n), batch_size=batch_size, shuffle=shuffle, collate_fn=list)


class EpochBook:
    """The device record of one ``train()`` (``hmp_epoch_ctl``), its per-epoch log and the segment table of the best-state
    snapshot.  ``tensors``: the model state to snapshot, contiguous device tensors (at most 64); the snapshot starts as a copy of
    them.  Nothing but :meth:`read` and :meth:`status` synchronises."""

    def __init__(self, device, log_cap: int, tensors: Sequence[torch.Tensor] = (), grid_blocks: Optional[int] = None):
        self.lib = _lib.require_device()
        self.device = torch.device(device)
        if len(tensors) > _lib.EPOCH_MAX_SEGS:
            raise _lib.HydraMPError(f"the model state has {len(tensors)} tensors; the snapshot table holds {_lib.EPOCH_MAX_SEGS}")
        for t in tensors:
            if not t.is_cuda or not t.is_contiguous():
                raise _lib.HydraMPError("EpochBook: the model state must be contiguous device tensors")
        self.log_cap = int(log_cap)
        self.ctl = torch.zeros(C.sizeof(_lib.EpochCtl), dtype=torch.uint8, device=self.device)
        self.log = torch.zeros(max(self.log_cap, 1) * C.sizeof(_lib.EpochRow), dtype=torch.uint8, device=self.device)
        self.tensors = list(tensors)
        self.snapshot = [t.detach().clone() for t in self.tensors]
        self.n_segs = len(self.tensors)
        segs = (_lib.EpochSeg * max(self.n_segs, 1))()
        total = 0
        for i, (s, d) in enumerate(zip(self.tensors, self.snapshot)):
            nbytes = s.numel() * s.element_size()
            segs[i] = _lib.EpochSeg(s.data_ptr(), d.data_ptr(), nbytes)
            total += nbytes
        self.segs = torch.frombuffer(bytearray(bytes(segs)), dtype=torch.uint8).to(self.device)
        # one 16-byte unit per thread and pass, 256 threads per workgroup, at most 256 workgroups
        self.grid_blocks = int(grid_blocks) if grid_blocks else max(1, min(256, (total // 16 + 255) // 256))

    def accumulate(self, loss: torch.Tensor, loss_count: Optional[torch.Tensor] = None, weight_tensor: Optional[torch.Tensor] = None,
                   weight: float = -1.0) -> None:
        """``loss`` / ``loss_count``: device float32 scalars (or views whose first element is read); ``weight_tensor``: device
        int64 scalar; see ``hmp_epoch_accumulate``"""
        _lib.check(self.lib.hmp_epoch_accumulate(self.ctl.data_ptr(), loss.data_ptr(),
                                                 loss_count.data_ptr() if loss_count is not None else None,
                                                 weight_tensor.data_ptr() if weight_tensor is not None else None, float(weight),
                                                 _lib.stream_ptr()))

    def close(self, counts: torch.Tensor, loss_div: float = 0.0, min_log_epoch: int = 0, early_stop_window: int = -1) -> None:
        n = int(counts.numel())
        if counts.dtype != torch.int64 or n not in (2, 4) or not counts.is_contiguous() or counts.device != self.device:
            raise _lib.HydraMPError("EpochBook.close: counts must be a contiguous device int64[2] or int64[4] tensor")
        _lib.check(self.lib.hmp_epoch_close(self.ctl.data_ptr(), self.log.data_ptr(), self.log_cap, counts.data_ptr(), n,
                                            float(loss_div), int(min_log_epoch), int(early_stop_window), self.segs.data_ptr(),
                                            self.n_segs, self.grid_blocks, _lib.stream_ptr()))

    def restore(self) -> None:
        _lib.check(self.lib.hmp_epoch_restore(self.segs.data_ptr(), self.n_segs, self.grid_blocks, _lib.stream_ptr()))

    def read(self) -> Tuple[_lib.EpochCtl, List[_lib.EpochRow]]:
        """the record and the rows of the epochs closed so far (synchronises)"""
        ctl = _lib.EpochCtl()
        rows = (_lib.EpochRow * max(self.log_cap, 1))()
        n = C.c_int32()
        _lib.check(self.lib.hmp_epoch_read(self.ctl.data_ptr(), self.log.data_ptr(), self.log_cap, C.byref(ctl), rows, C.byref(n),
                                           _lib.stream_ptr()))
        return ctl, [rows[i] for i in range(n.value)]

    def status(self) -> int:
        """the 4-byte status word (synchronises)"""
        st = C.c_int32()
        _lib.check(self.lib.hmp_epoch_read_status(self.ctl.data_ptr(), C.byref(st), _lib.stream_ptr()))
        return st.value


class BaseTrainingJob:
    def __init__(self, dataset_dict, network_params, double_precision=False):
        # data_type(): homogeneous | heterogeneous | homogeneous_htree | heterogeneous_htree
        self._set_types(dataset_dict["train"].data_type())
        self._dataset_dict = dataset_dict
        self._training_params = self.create_default_params()
        self._update_training_params(network_params=network_params)
        first = dataset_dict["train"].get_data(0)
        dim_key = "input_dim" if self._graph_type == "homogeneous" else "input_dim_dict"
        self._update_training_params(network_params={dim_key: first.num_node_features(), "output_dim": first.num_room_labels()})
        self._finish_init(double_precision)

    def _set_types(self, data_type: str) -> None:
        parts = data_type.split("_")
        self._network_type = "neural_tree" if len(parts) == 2 else "baseline"
        self._graph_type = parts[0]

    def _finish_init(self, double_precision: bool) -> None:
        self.clean_up_network_params()
        self._net = self.initialize_network()
        if double_precision:
            self._net.double()
        self._stores = {}

    @staticmethod
    def create_default_params():
        return {
            "network_params": {"hidden_dim": 32, "num_layers": 3, "dropout": 0.25, "conv_block": "GraphSAGE", "GAT_hidden_dims": 16,
                               "GAT_heads": [4, 4], "GAT_concats": [True, False], "ignored_label": 25},
            "optimization_params": {"lr": 0.01, "num_epochs": 200, "weight_decay": 0.001, "batch_size": 64, "shuffle": True},
        }

    def clean_up_network_params(self):
        params = self._training_params["network_params"]
        unused = ("num_layers", "hidden_dim") if params["conv_block"][:3] == "GAT" else ("GAT_hidden_dims", "GAT_heads", "GAT_concats")
        for key in unused:
            params.pop(key)

    def print_training_params(self, f=sys.stdout):
        for group, values in self._training_params.items():
            print(group, file=f)
            for name, value in values.items():
                print("   {}: {}".format(name, value), file=f)

    def _update_training_params(self, network_params=None, optimization_params=None):
        for group, new in (("network_params", network_params), ("optimization_params", optimization_params)):
            if new is not None:
                self._training_params[group].update(new)

    def initialize_network(self):
        classes = {("homogeneous", "baseline"): HomogeneousNetwork, ("homogeneous", "neural_tree"): HomogeneousNeuralTreeNetwork,
                   ("heterogeneous", "baseline"): HeterogeneousNetwork,
                   ("heterogeneous", "neural_tree"): HeterogeneousNeuralTreeNetwork}
        cls = classes[("homogeneous" if self._graph_type == "homogeneous" else "heterogeneous", self._network_type)]
        return cls(**self._training_params["network_params"])

    def get_network_params(self):
        return self._training_params["network_params"]

    def train_job_type(self):
        return f"{self._graph_type} {self._network_type}"

    def get_dataset(self, split_name):
        return self._dataset_dict[split_name]

    def ignored_label(self):
        return self._training_params["network_params"]["ignored_label"]

    # ---- device plumbing ---------------------------------------------------------------------------------------------------
    def _device(self, gpu_index: int) -> torch.device:
        assert gpu_index >= 0
        _lib.require_device()  # no device: HydraMPError (there is no CPU fallback)
        return torch.device(f"cuda:{gpu_index}" if gpu_index < torch.cuda.device_count() else "cuda:0")

    def _op_path(self) -> bool:
        return bool(getattr(self._net, "op_path", False))

    def _streams_batches(self) -> bool:
        """the fused step runs on BatchStream batches: every GraphSAGE / GAT / GAT_edge model, both tasks"""
        return not self._op_path()

    def _label_type(self) -> str:
        if self._graph_type == "homogeneous":
            from .store import HOMO_NODE

            return HOMO_NODE
        return "rooms" if self._network_type == "baseline" else "room_virtual"

    def _store(self, name, dataset, device):
        from .store import GraphStore, StoreDataset

        if isinstance(dataset, StoreDataset):  # already resident: the dataset's own store, no host graphs in between
            if dataset.store.device != device:
                raise _lib.HydraMPError(f"the StoreDataset's store lives on {dataset.store.device}, the job runs on {device}")
            if self._stores.get(name) is None or self._stores[name][1] is not dataset:
                self._stores[name] = (dataset.store, dataset, {})
            return dataset.store
        hit = self._stores.get(name)
        if hit is None or hit[0].device != device or hit[1] is not dataset:
            hit = (GraphStore([dataset[i] for i in range(len(dataset))], device), dataset, {})
            self._stores[name] = hit
        return hit[0]

    def _stream(self, name, dataset, device, batch_size):
        store = self._store(name, dataset, device)
        cache = self._stores[name][2]
        key = (id(self._net.native()), int(batch_size))
        if key not in cache:
            cache.clear()
            cache[key] = self._new_stream(store, batch_size)
        return cache[key]

    def _new_stream(self, store, batch_size):
        return store.stream(self._net, batch_size, self._label_type(), ignored_label=self.ignored_label())

    def _state_tensors(self) -> List[torch.Tensor]:
        """what ``deepcopy(net.state_dict())`` holds: the flat parameter buffer of a native net (its named parameters are views of
        it), every parameter and buffer of a GCN / GIN model"""
        net = self._net
        if not self._op_path():
            return [net.native().flat_params()]
        if getattr(net, "pre_mp", None) is not None:
            net.native().flat_params()  # re-homes pre_mp's parameters into their flat buffer before addresses are taken
        return [t for t in net.state_dict().values()]

    # ---- the loop bodies ---------------------------------------------------------------------------------------------------
    def _room_labels(self, batch) -> torch.Tensor:
        if self._graph_type == "homogeneous":
            return batch.y[batch.room_mask]
        return batch[self._label_type()].y

    def _class_weight(self, device, opt_params):
        """``optimization_params["class_weight"]`` resolved for the room head: None, or a float32 device vector -- "balanced" from
        the training split's resident store, explicit weights as they are"""
        from .models.utils import class_weight_tensor

        spec = opt_params.get("class_weight")
        if spec is None:
            return None
        C = evaluate._n_classes(self._net)
        if isinstance(spec, str):
            from .store import check_weight_scheme

            check_weight_scheme(spec)
            store = self._store("train", self.get_dataset("train"), device)
            label_type = "rooms" if store.homogeneous else self._label_type()
            return store.class_weights(label_type, n_classes=C, ignored_label=self.ignored_label(), scheme=spec)
        return class_weight_tensor(spec, C, device, 'optimization_params["class_weight"]')

    def _make_trainer(self, device, opt_params):
        """(train_batch(ids, book), count_batch(split, ids, counts, confusion), set_lr(lr)) for the room task"""
        net, ignored = self._net, self.ignored_label()
        B = opt_params["batch_size"]
        lr, wd = opt_params["lr"], opt_params["weight_decay"]
        cw = self._class_weight(device, opt_params)
        if self._streams_batches():
            streams = {s: self._stream(s, self.get_dataset(s), device, B) for s in ("train", "val", "test")}
            step = net.train_step(lr=lr, weight_decay=wd, ignored_label=ignored, use_graph=False, class_weight=cw)
            tail = step.grads[net.native().n_active:]

            def train_batch(ids, book):
                step.run(streams["train"].next(ids))
                book.accumulate(tail, tail[1:])  # {loss_sum, count}: weight = the valid-label count (weighted: the sum of weights)

            def count_batch(split, ids, counts, confusion=None):
                net.count_correct_rooms(streams[split].next(ids), counts, confusion, ignored)

            return train_batch, count_batch, step.set_lr
        stores = {s: self._store(s, self.get_dataset(s), device) for s in ("train", "val", "test")}

        def count_batch(split, ids, counts, confusion=None):
            net.count_correct_rooms(stores[split].collate(ids), counts, confusion, ignored)

        opt = torch.optim.Adam(net.parameters(), lr=lr, weight_decay=wd)

        def train_batch(ids, book):  # GCN / GIN: the reference's body
            b = stores["train"].collate(ids)
            opt.zero_grad()
            pred = net(b)
            label = self._room_labels(b)
            mask = label != ignored
            loss = net.loss(pred, label, mask, weight=cw)
            loss.backward()
            opt.step()
            if cw is None:
                book.accumulate(loss.detach(), None, mask.sum())
            else:  # {weighted sum, sum of weights}, as the fused step's tail: the epoch's loss is their ratio over the epoch
                ws = (cw[label.clamp(0, cw.numel() - 1)] * (mask & (label >= 0) & (label < cw.numel()))).sum()
                pair = torch.stack([loss.detach() * ws, ws])
                book.accumulate(pair, pair[1:])

        def set_lr(value):
            for group in opt.param_groups:
                group["lr"] = value

        return train_batch, count_batch, set_lr

    N_COUNTS = 2

    def _loss_div(self) -> float:
        return 0.0  # the epoch's loss is divided by the sum of the weights (the valid labels, :220)

    def _split_sizes(self):
        return {s: len(self.get_dataset(s)) for s in ("train", "val", "test")}

    TRAIN_SPLIT, VAL_SPLIT, TEST_SPLIT = "train", "val", "test"

    def _run_loop(self, log_folder, opt_params, decay_epochs, decay_rate, early_stop_window, min_log_epoch, verbose, device):
        net = self._net
        net.to(device)
        print(f"Training on GPU {device.index}.")
        B, num_epochs, lr = opt_params["batch_size"], opt_params["num_epochs"], opt_params["lr"]
        with torch.cuda.device(device):
            train_batch, count_batch, set_lr = self._make_trainer(device, opt_params)
            sizes = self._split_sizes()
            loader = order_loader(sizes[self.TRAIN_SPLIT], B, opt_params["shuffle"])
            val_ids = id_chunks(sizes[self.VAL_SPLIT], B)
            book = EpochBook(device, num_epochs, self._state_tensors())
            counts = torch.zeros(self.N_COUNTS, dtype=torch.int64, device=device)
            loss_div = self._loss_div()

            tic = time.perf_counter()
            for epoch in range(num_epochs):
                set_lr(lr * decay_rate ** (epoch // decay_epochs))  # StepLR(step_size=decay_epochs, gamma=decay_rate)
                net.train()
                for ids in loader:
                    train_batch(ids, book)
                if verbose:
                    train_result = self._pass_accuracy(count_batch, self.TRAIN_SPLIT, id_chunks(sizes[self.TRAIN_SPLIT], B), device)
                net.eval()
                for ids in val_ids:
                    count_batch(self.VAL_SPLIT, ids, counts)
                book.close(counts, loss_div, min_log_epoch, early_stop_window)
                if verbose and (epoch + 1) % 10 == 0:
                    row = book.read()[1][-1]
                    print("Epoch {:03}. Loss: {:.4f}. Train accuracy: {:.4f}. Validation accuracy: {:.4f}.".format(
                        epoch, row.loss, train_result, row.val_acc))
                if early_stop_window >= 0 and book.status() & _lib.EPOCH_STOP:
                    if verbose:
                        print("Early stopping condition reached at {} epoch.".format(epoch))
                    break
            book.restore()  # the best state back into the model (a no-change copy when no epoch improved)
            ctl, rows = book.read()
            toc = time.perf_counter()
        print("Training completed (time elapsed: {:.4f} s). ".format(toc - tic))
        info = {"training_time": toc - tic, "num_epochs": int(ctl.epoch), "best_epoch": int(ctl.best_epoch),
                "loss": [r.loss for r in rows], "validation_result": [r.val_acc for r in rows]}
        self._write_scalars(log_folder, rows)
        if ctl.status & _lib.EPOCH_EMPTY_VAL:
            raise ZeroDivisionError("a validation pass counted no labelled row (correct / total with total == 0)")
        if not any(r.improved for r in rows):
            raise _lib.HydraMPError("no epoch improved on a validation accuracy of 0: there is no best state to load")
        return float(ctl.max_val_acc), info, count_batch

    def _pass_accuracy(self, count_batch, split, id_lists, device) -> float:
        c = torch.zeros(self.N_COUNTS, dtype=torch.int64, device=device)
        for ids in id_lists:
            count_batch(split, ids, c)
        c = c.cpu().tolist()  # the one synchronisation of the pass
        return sum(c[0::2]) / sum(c[1::2])

    @staticmethod
    def _write_scalars(log_folder, rows) -> None:
        os.makedirs(log_folder, exist_ok=True)
        series = {"loss": [r.loss for r in rows], "validation result": [r.val_acc for r in rows]}
        try:
            from tensorboardX import SummaryWriter
        except ImportError:
            with open(os.path.join(log_folder, "scalars.json"), "w") as f:
                json.dump(series, f)
            return
        writer = SummaryWriter(log_folder)
        for name, values in series.items():
            for epoch, value in enumerate(values):
                writer.add_scalar(name, value, epoch)
        writer.close()

    def train(self, log_folder, optimization_params=None, decay_epochs=100, decay_rate=1.0, early_stop_window=-1, min_log_epoch=0,
              verbose=False, gpu_index=0):
        """``BaseTrainingJob.train`` (:131-267): returns ``(net, (max_val_acc, test_result), info)`` with the best state loaded.
        ``info`` carries the reference's ``training_time`` / ``num_epochs`` / ``test_time`` plus ``best_epoch`` and the per-epoch
        ``loss`` / ``validation_result`` series of the device log.  Raises ``HydraMPError`` without a gfx950 device."""
        device = self._device(gpu_index)
        self._update_training_params(optimization_params=optimization_params)
        opt_params = self._training_params["optimization_params"]
        max_val_acc, info, count_batch = self._run_loop(log_folder, opt_params, decay_epochs, decay_rate, early_stop_window,
                                                        min_log_epoch, verbose, device)
        tic = time.perf_counter()
        with torch.cuda.device(device):
            test_result = self._final_test(count_batch, opt_params["batch_size"], device)
        toc = time.perf_counter()
        print("Testing completed (time elapsed: {:.4f} s). ".format(toc - tic))
        print("Best validation accuracy: {:.4f}, corresponding test accuracy: {:.4f}.".format(max_val_acc, test_result))
        info["test_time"] = toc - tic
        torch.cuda.empty_cache()
        return self._net, (max_val_acc, test_result), info

    def _final_test(self, count_batch, batch_size, device) -> float:
        self._net.eval()
        n = self._split_sizes()[self.TEST_SPLIT]
        return self._pass_accuracy(count_batch, self.TEST_SPLIT, id_chunks(n, batch_size), device)

    def test(self, data_loader, get_per_label_accuracy=False, get_balanced_accuracy=False):
        """``BaseTrainingJob.test`` (:269-313) with one synchronisation per pass.  ``data_loader``: a split name (``"train"`` /
        ``"val"`` / ``"test"``: the job's own device-resident copy, in ``batch_size`` batches) or an iterable of batches.
        ``get_balanced_accuracy=True`` appends the mean per-class recall (``evaluate.accuracy(..., balanced=True)``)."""
        net = self._net
        net.eval()
        device = next(net.parameters()).device
        if isinstance(data_loader, str):
            dataset = self.get_dataset(data_loader)
            B = self._training_params["optimization_params"]["batch_size"]
            with torch.cuda.device(device):
                if self._streams_batches():
                    batches = (self._stream(data_loader, dataset, device, B), id_chunks(len(dataset), B))
                else:
                    store = self._store(data_loader, dataset, device)
                    batches = (store.collate(ids) for ids in id_chunks(len(dataset), B))
                return evaluate.accuracy(net, batches, self.ignored_label(), get_per_label_accuracy, get_balanced_accuracy)
        return evaluate.accuracy(net, (b.to(device) for b in data_loader), self.ignored_label(), get_per_label_accuracy,
                                 get_balanced_accuracy)

    def predict(self, split):
        """Predicted labels of every graph of the split ``"train"`` / ``"val"`` / ``"test"``, from the job's own device-resident copy
        in ``batch_size`` batches with one device-to-host copy per pass (``evaluate.predict``): a list with one numpy int64 array
        per graph, the labels ``model.predict`` returns for that graph alone."""
        return self._predict_pass(split, self.get_dataset(split))

    def predict_topk(self, split, k):
        """:meth:`predict` with the top-k labels and their softmax probabilities (``evaluate.predict_topk``): per graph
        ``(labels [n, k] int64, probs [n, k] float32)`` numpy arrays over the rows :meth:`predict` returns (``labels[:, 0]`` is its
        result), or a ``(room, object)`` pair of those for a two-headed model; one device-to-host copy per pass."""
        return self._predict_pass(split, self.get_dataset(split), k)

    def predict_mc(self, split, samples):
        """:meth:`predict` with Monte-Carlo dropout uncertainty over ``samples`` stochastic passes (``evaluate.predict_mc``, the
        model's dropout seed): per graph ``(labels [n] int64, mean_probs [n, C], std [n], entropy [n], mutual_info [n] float32)``
        numpy arrays over the rows :meth:`predict` returns, or a ``(room, object)`` pair of those for a two-headed model; one
        device-to-host copy per pass."""
        return self._predict_pass(split, self.get_dataset(split), mc=samples)

    def saliency(self, split, groups=((0, 3), (3, 6), (6, None)), **kw):
        """Gradient saliency of every graph of the split ``"train"`` / ``"val"`` / ``"test"``, from the job's own device-resident copy
        in ``batch_size`` batches with one device-to-host copy per pass (``evaluate.saliency``): per graph ``{node_type: (gxi [n],
        gnorm [n], groups [n, n_groups])}`` numpy arrays (homogeneous models: the one triple) of the gradient of the rows' own
        predicted-class logits.  GraphSAGE / GAT / GAT_edge models; GCN / GIN models are refused by name."""
        net = self._net
        if self._op_path():
            raise _lib.HydraMPError(f"saliency: {net.conv_block} models run op by op (hydra_gnn_amd.ops), not the native program: they "
                                    "have no input-gradient path (GraphSAGE, GAT and GAT_edge models do)")
        net.eval()
        dataset = self.get_dataset(split)
        device = next(net.parameters()).device
        B = self._training_params["optimization_params"]["batch_size"]
        with torch.cuda.device(device):
            return evaluate.saliency(net, (self._stream(split, dataset, device, B), id_chunks(len(dataset), B)), groups=groups, **kw)

    def _predict_pass(self, name, dataset, k=None, mc=None):
        """``k`` None: the labels of ``evaluate.predict``; else the top-k pairs of ``evaluate.predict_topk``.  ``mc``: the sample
        count of ``evaluate.predict_mc`` instead"""
        net = self._net
        net.eval()
        device = next(net.parameters()).device
        B = self._training_params["optimization_params"]["batch_size"]
        chunks = id_chunks(len(dataset), B)
        run = evaluate.predict if k is None else (lambda model, batches: evaluate.predict_topk(model, batches, k))
        if mc is not None:
            run = lambda model, batches: evaluate.predict_mc(model, batches, mc)  # noqa: E731
        with torch.cuda.device(device):
            if self._streams_batches():
                return run(net, (self._stream(name, dataset, device, B), chunks))
            # GCN / GIN: collated batches keep no graph offsets; the per-node vectors are split by the store's node counts
            store = self._store(name, dataset, device)
            per_batch = run(net, (store.collate(ids) for ids in chunks))
        nodes = store.node_counts[store.node_types[0]]
        out = []
        for ids, labels in zip(chunks, per_batch):
            two = isinstance(labels if (k is None and mc is None) else labels[0], tuple)
            if mc is not None:
                heads = [evaluate._split_mc(list(hd), nodes[ids]) for hd in (labels if two else (labels,))]
            elif k is None:
                heads = [evaluate._split_rows(v, nodes[ids]) for v in (labels if two else (labels,))]
            else:
                heads = [evaluate._split_topk(lb, pb, nodes[ids]) for lb, pb in (labels if two else (labels,))]
            out.extend(zip(*heads) if two else heads[0])
        return out

    def test_individual_graph(self, dataset, model=None):
        """``(correct, total)`` of every graph of ``dataset`` (:315-339): the dataset is uploaded once (and kept, like the splits),
        counted in ``batch_size`` batches with one forward and one per-graph count launch each
        (``count_correct_rooms_per_graph``), and read once"""
        if model is not None:
            self._net = model
        net = self._net
        net.eval()
        device = next(net.parameters()).device
        if not hasattr(dataset, "__getitem__"):
            dataset = list(dataset)
        n = len(dataset)
        if n == 0:
            return []
        B = self._training_params["optimization_params"]["batch_size"]
        ignored = self.ignored_label()
        with torch.cuda.device(device):
            counts = torch.zeros(n, 2, dtype=torch.int64, device=device)
            if self._streams_batches():
                stream = self._stream("individual", dataset, device, B)
                for ids in id_chunks(n, B):
                    net.count_correct_rooms_per_graph(stream.next(ids), counts[ids[0]:ids[-1] + 1], ignored)
            else:  # GCN / GIN (homogeneous): a collated Data keeps no ptr, the node offsets come from the store's counts
                store = self._store("individual", dataset, device)
                nodes = torch.from_numpy(store.node_counts[store.node_types[0]])
                for ids in id_chunks(n, B):
                    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), nodes[ids[0]:ids[-1] + 1].cumsum(0)]).to(device)
                    net.count_correct_rooms_per_graph(store.collate(ids), counts[ids[0]:ids[-1] + 1], ignored, graph_ptr=ptr)
            return [(int(c), int(t)) for c, t in counts.cpu().tolist()]  # the one synchronisation


class SemiSupervisedTrainingJob(BaseTrainingJob):
    """The two-headed (room + object) job over ONE dataset whose graphs carry ``train_mask`` / ``val_mask`` / ``test_mask``."""

    def __init__(self, dataset, network_params, double_precision=False):
        self._set_types(dataset.data_type())
        self._dataset = dataset
        self._training_params = self.create_default_params()
        self._update_training_params(network_params=network_params)
        first = dataset.get_data(0)
        dim_key = "input_dim" if self._graph_type == "homogeneous" else "input_dim_dict"
        if self._network_type == "baseline":
            out = {"rooms": first.num_room_labels(), "objects": first.num_object_labels()}
        else:
            out = {"room": first.num_room_labels(), "object": first.num_object_labels(), "object-room": 1, "room-room": 1}
        self._update_training_params(network_params={dim_key: first.num_node_features(), "output_dim_dict": out})
        self._finish_init(double_precision)

    def get_dataset(self, split_name=None):
        return self._dataset

    N_COUNTS = 4
    TRAIN_SPLIT = VAL_SPLIT = TEST_SPLIT = "all"

    def _split_sizes(self):
        return {"all": len(self._dataset)}

    def _loss_div(self) -> float:
        return float(len(self._dataset))  # total_loss /= len(data_loader.dataset) (:149)

    def _new_stream(self, store, batch_size):
        return store.stream(self._net, batch_size)

    def _targets(self, batch, mask_name):
        """(labels, masks) of (rooms, objects) as the reference picks them (:121-143, :220-242)"""
        if self._graph_type == "homogeneous":
            rows = (batch.room_mask, ~batch.room_mask if self._network_type == "baseline" else batch.object_mask)
            m = getattr(batch, mask_name)
            return tuple(batch.y[r] for r in rows), tuple(m[r] for r in rows)
        types = ("rooms", "objects") if self._network_type == "baseline" else ("room_virtual", "object_virtual")
        return tuple(batch[t].y for t in types), tuple(getattr(batch[t], mask_name) for t in types)

    def _count_op_path(self, batch, mask_name, counts) -> None:
        """GCN / GIN: the arithmetic of ``test()`` (:216-253) added into the device int64[4] ``counts`` without a host read"""
        with torch.no_grad():
            pred = self._net(batch)
            label, mask = self._targets(batch, mask_name)
            for k, (p, l, m) in enumerate(zip(pred, label, mask)):
                counts[2 * k] += p.argmax(dim=1)[m].eq(l[m]).sum()
                counts[2 * k + 1] += m.sum()

    def _head_classes(self) -> Tuple[int, int]:
        net = self._net
        if self._op_path():
            return int(net.post_mp_room.out_features), int(net.post_mp_object.out_features)
        return tuple(net.native().head_classes())

    def _class_weight(self, device, opt_params):
        """``optimization_params["class_weight"]`` resolved per head: None, or a pair (rooms, objects) of float32 device vectors
        / None -- "balanced" from the rows of ``train_mask`` in the resident store, explicit weights as they are"""
        from .models.utils import class_weight_tensor
        from .store import check_weight_scheme

        spec = opt_params.get("class_weight")
        if spec is None:
            return None
        if isinstance(spec, dict):
            unknown = set(spec) - {"rooms", "objects"}
            if unknown:
                raise _lib.HydraMPError(f'optimization_params["class_weight"]: the heads are "rooms" and "objects", got {sorted(unknown)}')
            per_head = [spec.get("rooms"), spec.get("objects")]
        elif isinstance(spec, str):
            per_head = [spec, spec]
        else:
            if isinstance(spec, torch.Tensor) or len(spec) != 2:
                raise _lib.HydraMPError('optimization_params["class_weight"]: the two-headed job takes "balanced", a pair or a dict '
                                        '{"rooms": ..., "objects": ...}')
            per_head = list(spec)
        store = self._store("all", self._dataset, device)
        if store.homogeneous:
            types = ("rooms", "objects")
        else:
            types = ("rooms", "objects") if self._network_type == "baseline" else ("room_virtual", "object_virtual")
        out = []
        for name, w, t, C in zip(("rooms", "objects"), per_head, types, self._head_classes()):
            if isinstance(w, str):
                check_weight_scheme(w)
                w = store.class_weights(t, mask="train_mask", n_classes=C, ignored_label=-100, scheme=w)
            elif w is not None:
                w = class_weight_tensor(w, C, device, f'optimization_params["class_weight"][{name}]')
            out.append(w)
        return None if all(w is None for w in out) else tuple(out)

    def _make_trainer(self, device, opt_params):
        net = self._net
        B, lr, wd = opt_params["batch_size"], opt_params["lr"], opt_params["weight_decay"]
        hetero = self._graph_type != "homogeneous"
        self._pass_mask = "val_mask"  # mask of the counting passes: val during the loop, train (verbose) / test around it
        cw = self._class_weight(device, opt_params)
        if self._streams_batches():
            stream = self._stream("all", self._dataset, device, B)
            step = net.semisupervised_step(lr=lr, weight_decay=wd, use_graph=False, class_weight=cw)
            tail = step.grads[net.native().n_active:]

            def train_batch(ids, book):
                step.run(stream.next(ids), mask="train_mask")
                book.accumulate(tail, tail[1:], None, float(len(ids)))  # loss.item() * batch.num_graphs (:148)

            def count_batch(split, ids, counts, confusion=None):
                if hetero:
                    net.count_correct(stream.next(ids), None, self._pass_mask, counts)
                else:
                    net.count_correct(stream.next(ids), self._pass_mask, counts)

            return train_batch, count_batch, step.set_lr
        store = self._store("all", self._dataset, device)
        opt = torch.optim.Adam(net.parameters(), lr=lr, weight_decay=wd)

        def train_batch(ids, book):
            b = store.collate(ids)
            opt.zero_grad()
            pred = net(b)
            label, mask = self._targets(b, "train_mask")
            loss = net.loss(pred, label, mask, weight=cw)
            loss.backward()
            opt.step()
            book.accumulate(loss.detach(), None, None, float(len(ids)))

        def count_batch(split, ids, counts, confusion=None):
            was = net.training
            net.eval()
            self._count_op_path(store.collate(ids), self._pass_mask, counts)
            net.train(was)

        def set_lr(value):
            for group in opt.param_groups:
                group["lr"] = value

        return train_batch, count_batch, set_lr

    def _pass_accuracy(self, count_batch, split, id_lists, device) -> float:
        # the verbose training-accuracy pass of the loop counts under train_mask (:156)
        self._pass_mask, was = "train_mask", self._pass_mask
        try:
            return super()._pass_accuracy(count_batch, split, id_lists, device)
        finally:
            self._pass_mask = was

    def _final_test(self, count_batch, batch_size, device) -> float:
        """the reference's one-batch test loader, counted in ``batch_size`` chunks (eval mode has no batch dependence)"""
        self._net.eval()
        self._pass_mask = "test_mask"
        return BaseTrainingJob._pass_accuracy(self, count_batch, "all", id_chunks(len(self._dataset), batch_size), device)

    def train(self, log_folder, optimization_params=None, decay_epochs=100, decay_rate=1.0, early_stop_window=-1, min_log_epoch=0,
              verbose=False, gpu_index=0):
        """``SemiSupervisedTrainingJob.train`` (:57-196): as :meth:`BaseTrainingJob.train`, on the masks of one dataset; the
        epoch's loss is ``sum(loss * num_graphs) / len(dataset)``, the accuracies sum rooms and objects."""
        return super().train(log_folder, optimization_params, decay_epochs, decay_rate, early_stop_window, min_log_epoch, verbose,
                             gpu_index)

    def test(self, data_loader=None, mask_name="test_mask", get_type_separated_accuracy=False):
        """``SemiSupervisedTrainingJob.test`` (:198-258) with one synchronisation per pass.  ``data_loader``: None = the job's
        dataset from its device-resident copy in ``batch_size`` batches, or an iterable of batches."""
        assert mask_name in ["train_mask", "val_mask", "test_mask"]
        net = self._net
        net.eval()
        device = next(net.parameters()).device
        B = self._training_params["optimization_params"]["batch_size"]
        with torch.cuda.device(device):
            if self._op_path():
                if data_loader is None:
                    store = self._store("all", self._dataset, device)
                    data_loader = (store.collate(ids) for ids in id_chunks(len(self._dataset), B))
                counts = torch.zeros(4, dtype=torch.int64, device=device)
                for b in data_loader:
                    self._count_op_path(b.to(device), mask_name, counts)
                cr, tr, co, to = counts.cpu().tolist()  # the one synchronisation of the pass
                return (cr / tr, co / to) if get_type_separated_accuracy else (cr + co) / (tr + to)
            if data_loader is None:
                batches = (self._stream("all", self._dataset, device, B), id_chunks(len(self._dataset), B))
            else:
                batches = (b.to(device) for b in data_loader)
            return evaluate.semisupervised_accuracy(net, batches, mask_name, get_type_separated_accuracy)

    def predict(self, split=None):
        """Predicted ``(room_labels, object_labels)`` of every graph of the job's dataset (one pair of numpy int64 arrays per graph,
        what ``model.predict`` returns for that graph alone), from its device-resident copy in ``batch_size`` batches with one
        device-to-host copy per pass."""
        return self._predict_pass("all", self._dataset)

    def predict_topk(self, k, split=None):
        """:meth:`predict` with the top-k labels and their softmax probabilities: per graph
        ``((room_labels [n, k], room_probs [n, k]), (object_labels, object_probs))`` numpy arrays (``evaluate.predict_topk``)."""
        return self._predict_pass("all", self._dataset, k)

    def predict_mc(self, samples, split=None):
        """:meth:`predict` with Monte-Carlo dropout uncertainty over ``samples`` stochastic passes: per graph a ``(room, object)``
        pair of ``(labels [n], mean_probs [n, C], std [n], entropy [n], mutual_info [n])`` numpy arrays (``evaluate.predict_mc``)."""
        return self._predict_pass("all", self._dataset, mc=samples)

    def test_individual_graph(self, dataset, model=None):
        return NotImplemented
