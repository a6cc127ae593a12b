"""Validation accuracy on the device (room task: :func:`accuracy`; two-headed task: :func:`semisupervised_accuracy`): ``BaseTrainingJob.test`` (``base_training_job.py:269-313``) without a sync
per batch.

The reference's ``test()`` runs an eval-mode forward per batch, takes ``argmax(dim=1)``, drops the rows whose label is the
``ignored_label`` and adds ``pred.eq(label).sum().item()`` -- a device-to-host round trip per batch.  :func:`accuracy` runs
``model.count_correct_rooms`` per batch instead (eval-mode native forward + one count launch, ``hmp_net_count_correct_rooms``),
which adds {correct, total} and, with ``per_label=True``, the confusion matrix into device int64 accumulators, and reads them
ONCE at the end of the pass.

    acc = evaluate.accuracy(model, val_batches)                            # batches already on the device
    acc = evaluate.accuracy(model, (stream, id_lists))                     # store.BatchStream + graph ids per batch
    acc, matrix = evaluate.accuracy(model, val_batches, per_label=True)    # test(loader, get_per_label_accuracy=True)

The per-label matrix is the reference's ``(C - 1) x C`` int array (``accuracy_matrix[l, p]`` = rows of label ``l`` predicted
as ``p``; the ``ignored_label`` row stays zero), summed over the pass.  The reference's loop ASSIGNS each batch's matrix, so
its result is the last batch's; the two agree for a loader that yields one batch.
"""
from __future__ import annotations

from typing import Iterable, Tuple, Union

import numpy as np
import torch


def accuracy_matrix(confusion, ignored_label: int = 25) -> np.ndarray:
    """The reference's ``(C - 1) x C`` ``accuracy_matrix`` (``base_training_job.py:275-278,297-308``) from a ``[C, C]`` (or
    ``[C * C]``) confusion matrix ``confusion[label, pred]``: rows ``l < C - 1`` except ``l == ignored_label``, every column."""
    conf = confusion.detach().cpu().numpy() if isinstance(confusion, torch.Tensor) else np.asarray(confusion)
    C = int(round(np.sqrt(conf.size)))
    if C * C != conf.size:
        raise ValueError(f"confusion matrix of {conf.size} entries is not square")
    conf = conf.reshape(C, C)
    out = np.zeros((C - 1, C), dtype=int)
    for l in range(C - 1):
        if l != ignored_label:
            out[l] = conf[l]
    return out


def _n_classes(model) -> int:
    op_path = getattr(model, "op_path", False)
    if op_path:  # GCN / GIN: the width of the last conv
        conv = model.convs[-1]
        return int((conv.nn[2] if model.conv_block == "GIN" else conv.lin).weight.size(0))
    return model.native().n_classes


def accuracy(model, batches: Union[Iterable, Tuple[object, Iterable]], ignored_label: int = 25, per_label: bool = False):
    """``correct / total`` of the room task over ``batches`` (``BaseTrainingJob.test``), accumulated on the device with ONE
    synchronisation at the end.  ``batches``: an iterable of batches on the model's device, or a ``(BatchStream, iterable of
    graph-id lists)`` pair.  With ``per_label=True`` returns ``(accuracy, accuracy_matrix)``."""
    from .store import BatchStream

    dev = next(model.parameters()).device
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    confusion = None
    if per_label:
        C = _n_classes(model)
        confusion = torch.zeros(C * C, dtype=torch.int64, device=dev)
    if isinstance(batches, tuple) and len(batches) == 2 and isinstance(batches[0], BatchStream):
        stream, id_lists = batches
        for ids in id_lists:
            model.count_correct_rooms(stream.next(ids), counts, confusion, ignored_label)
    else:
        for batch in batches:
            model.count_correct_rooms(batch, counts, confusion, ignored_label)
    # the one synchronisation of the pass
    host = (torch.cat([counts[:2], confusion]) if confusion is not None else counts[:2]).cpu()
    correct, total = int(host[0]), int(host[1])
    acc = correct / total  # the reference's division (a pass without labelled rows raises ZeroDivisionError there too)
    return (acc, accuracy_matrix(host[2:], ignored_label)) if per_label else acc


def semisupervised_accuracy(model, batches: Union[Iterable, Tuple[object, Iterable]], mask_name: str = "test_mask",
                            type_separated: bool = False):
    """The arithmetic of ``SemiSupervisedTrainingJob.test`` (``semisupervised_training_job.py:198-258``) for the two-headed
    (room + object) task with ONE synchronisation per pass: ``model.count_correct`` per batch adds {correct_room, total_room,
    correct_object, total_object} to one device int64[4] tensor, which is copied to the host after the last batch.

    ``batches``: an iterable of batches on the model's device (``HeteroData`` for the heterogeneous models, their labels and
    masks read from the node types of ``net.head_label_types()``; ``Data`` for the homogeneous ones), or a ``(BatchStream,
    iterable of graph-id lists)`` pair of a two-headed stream.  Returns ``(correct_room + correct_object) / (total_room +
    total_object)``, or with ``type_separated=True`` the pair ``(correct_room / total_room, correct_object / total_object)``."""
    from .store import BatchStream

    if mask_name not in ("train_mask", "val_mask", "test_mask"):  # the reference's assert (:201)
        raise ValueError(f"mask_name must be train_mask, val_mask or test_mask, got {mask_name!r}")
    dev = next(model.parameters()).device
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    hetero = model.native().aux_readout is not None
    if isinstance(batches, tuple) and len(batches) == 2 and isinstance(batches[0], BatchStream):
        stream, id_lists = batches
        for ids in id_lists:
            if hetero:
                model.count_correct(stream.next(ids), None, mask_name, counts)
            else:
                model.count_correct(stream.next(ids), mask_name, counts)
    else:
        types = model.native().head_label_types() if hetero else None
        for batch in batches:
            if hetero:
                model.count_correct(batch, tuple(batch[t].y for t in types), tuple(getattr(batch[t], mask_name) for t in types), counts)
            else:
                model.count_correct(batch, mask_name, counts)
    correct_room, total_room, correct_object, total_object = (int(v) for v in counts.cpu())  # the one synchronisation of the pass
    if type_separated:
        return correct_room / total_room, correct_object / total_object
    return (correct_room + correct_object) / (total_room + total_object)
