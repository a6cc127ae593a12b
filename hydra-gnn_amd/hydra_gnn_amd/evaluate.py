"""Validation accuracy on the device (room task: :func:`accuracy`; two-headed task: :func:`semisupervised_accuracy`) and the
predicted labels themselves (:func:`predict`, every model and task; :func:`predict_topk` adds the next guesses and the softmax
probability of each, :func:`predict_mc` the Monte-Carlo dropout mean, entropy and mutual information): ``BaseTrainingJob.test`` (``base_training_job.py:269-313``) without a sync
per batch.

The reference's ``test()`` runs an eval-mode forward per batch, takes ``argmax(dim=1)``, drops the rows whose label is the
``ignored_label`` and adds ``pred.eq(label).sum().item()`` -- a device-to-host round trip per batch.  :func:`accuracy` runs
``model.count_correct_rooms`` per batch instead (eval-mode native forward + one count launch, ``hmp_net_count_correct_rooms``),
which adds {correct, total} and, with ``per_label=True``, the confusion matrix into device int64 accumulators, and reads them
ONCE at the end of the pass.

    acc = evaluate.accuracy(model, val_batches)                            # batches already on the device
    acc = evaluate.accuracy(model, (stream, id_lists))                     # store.BatchStream + graph ids per batch
    acc, matrix = evaluate.accuracy(model, val_batches, per_label=True)    # test(loader, get_per_label_accuracy=True)
    acc, bal = evaluate.accuracy(model, val_batches, balanced=True)        # + mean per-class recall (balanced accuracy)

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


def balanced_accuracy(confusion) -> float:
    """Mean per-class recall over the classes with support, from a ``[C, C]`` (or ``[C * C]``) confusion matrix
    ``confusion[label, pred]``: ``mean_c conf[c, c] / sum_p conf[c, p]`` over the rows with a non-zero sum (scikit-learn's
    ``balanced_accuracy_score``).  The measure that class-weighted training moves; a matrix without any counted row raises
    ZeroDivisionError, as the plain accuracy of such a pass does."""
    conf = confusion.detach().cpu().numpy() if isinstance(confusion, torch.Tensor) else np.asarray(confusion)
    C = int(round(np.sqrt(conf.size)))
    if C * C != conf.size:
        raise ValueError(f"confusion matrix of {conf.size} entries is not square")
    conf = conf.reshape(C, C).astype(np.int64)
    support = conf.sum(axis=1)
    have = support > 0
    if not have.any():
        raise ZeroDivisionError("balanced accuracy of a pass without labelled rows")
    return float(np.mean(np.diag(conf)[have].astype(np.float64) / support[have].astype(np.float64)))


def _n_classes(model) -> int:
    op_path = getattr(model, "op_path", False)
    if op_path:  # GCN / GIN: the width of the last conv
        conv = model.convs[-1]
        return int((conv.nn[2] if model.conv_block == "GIN" else conv.lin).weight.size(0))
    return model.native().n_classes


def accuracy(model, batches: Union[Iterable, Tuple[object, Iterable]], ignored_label: int = 25, per_label: bool = False,
             balanced: bool = False):
    """``correct / total`` of the room task over ``batches`` (``BaseTrainingJob.test``), accumulated on the device with ONE
    synchronisation at the end.  ``batches``: an iterable of batches on the model's device, or a ``(BatchStream, iterable of
    graph-id lists)`` pair.  With ``per_label=True`` returns ``(accuracy, accuracy_matrix)``.  ``balanced=True`` appends the
    mean per-class recall over the classes with support (:func:`balanced_accuracy`) to the result, from the confusion counters
    the count launches fill anyway: no launch and no synchronisation more."""
    from .store import BatchStream

    dev = next(model.parameters()).device
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    confusion = None
    if per_label or balanced:
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
    out = (acc,) + ((accuracy_matrix(host[2:], ignored_label),) if per_label else ()) + ((balanced_accuracy(host[2:]),) if balanced else ())
    return out if len(out) > 1 else acc


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


def _label_types(model):
    """node types whose rows the label vectors of ``model.predict_labels`` follow: one per head"""
    nat = model.native()
    if nat.aux_readout is not None:
        return tuple(nat.head_label_types())
    out_type = nat.pool_edge_type[2] if nat.pool_edge_type is not None else nat.readout
    return (out_type, out_type) if nat.heads is not None else (out_type,)


def _split_rows(host: np.ndarray, counts: np.ndarray):
    """per-graph pieces of a label vector, the -1 rows (outside the head's rows) dropped"""
    off = np.concatenate([[0], np.cumsum(counts)])
    pieces = [host[off[g]:off[g + 1]] for g in range(len(counts))]
    return [p[p >= 0] for p in pieces]


def _pass_args(model, batches, who: str):
    """the two forms of ``batches`` checked: ``(stream, graph-id arrays)`` of a streamed pass, ``(None, None)`` for an iterable of
    batches"""
    from . import _lib
    from .store import BatchStream

    streamed = isinstance(batches, tuple) and len(batches) >= 1 and isinstance(batches[0], BatchStream)
    if streamed and len(batches) != 2:
        raise _lib.HydraMPError(f"{who}: a stream is passed as the pair (BatchStream, iterable of graph-id lists)")
    if batches is None or isinstance(batches, (str, bytes)) or not hasattr(batches, "__iter__"):
        raise _lib.HydraMPError(f"{who}: batches must be an iterable of batches or a (BatchStream, iterable of graph-id lists) pair")
    if not streamed:
        return None, None
    stream, id_lists = batches
    if id_lists is None or isinstance(id_lists, (str, bytes)) or not hasattr(id_lists, "__iter__"):
        raise _lib.HydraMPError(f"{who}: the second element of the pair must be an iterable of graph-id lists")
    id_lists = [np.asarray(ids, dtype=np.int64).reshape(-1) for ids in id_lists]
    if any(ids.size == 0 for ids in id_lists):
        raise _lib.HydraMPError(f"{who}: an empty graph-id list")
    if stream.nat is not model.native():
        raise _lib.HydraMPError(f"{who}: the stream was created for another model")
    return stream, id_lists


def predict(model, batches: Union[Iterable, Tuple[object, Iterable]]):
    """Predicted labels over ``batches`` with ONE device-to-host copy at the end of the pass (``model.predict_labels`` per batch:
    eval-mode forward plus one launch, nothing synchronises in between).  ``batches`` takes the two forms :func:`accuracy` takes.

    ``(BatchStream, iterable of graph-id lists)``: the label buffers of the whole pass are allocated once from the store's
    per-graph node counts, every batch writes its slice, and the result is a list with one entry per graph in id order -- a numpy
    int64 array (room task) or a ``(room, object)`` pair of arrays (two-headed), each what ``model.predict`` returns for that graph
    alone (the ``-1`` rows outside a head's rows are dropped on the host; the labels are a few KB, so nothing is compacted on the
    device).  An iterable of batches on the model's device: one entry per BATCH, the per-row vectors of ``predict_labels`` (``-1``
    rows kept: a collated homogeneous batch carries no graph offsets to split by)."""
    stream, id_lists = _pass_args(model, batches, "predict")
    streamed = stream is not None
    dev = next(model.parameters()).device
    if not streamed:
        outs = [model.predict_labels(b) for b in batches]
        two = bool(outs) and isinstance(outs[0], tuple)
        flat = [t for o in outs for t in (o if two else (o,))]
        if not flat:
            return []
        host = torch.cat(flat).cpu().numpy()  # the one copy of the pass
        sizes = np.cumsum([0] + [t.numel() for t in flat])
        parts = [host[sizes[i]:sizes[i + 1]] for i in range(len(flat))]
        return [(parts[2 * i], parts[2 * i + 1]) for i in range(len(outs))] if two else parts
    types = _label_types(model)
    two = len(types) == 2
    all_ids = np.concatenate(id_lists) if id_lists else np.zeros(0, dtype=np.int64)
    counts = [stream.store.node_counts[t][all_ids] for t in types]
    totals = [int(c.sum()) for c in counts]
    buf = torch.empty(max(sum(totals), 1), dtype=torch.int64, device=dev)  # head 0's rows of the whole pass, then head 1's
    pos = [0, totals[0]]
    for ids in id_lists:
        rows = [int(stream.store.node_counts[t][ids].sum()) for t in types]
        views = [buf[pos[k]:pos[k] + rows[k]] for k in range(len(types))]
        model.predict_labels(stream.next(ids), out=tuple(views) if two else views[0])
        for k in range(len(types)):
            pos[k] += rows[k]
    host = buf[:sum(totals)].cpu().numpy()  # the one copy (and synchronisation) of the pass
    heads = [_split_rows(host[:totals[0]], counts[0])]
    if two:
        heads.append(_split_rows(host[totals[0]:], counts[1]))
        return list(zip(heads[0], heads[1]))
    return heads[0]


def _split_topk(labels: np.ndarray, probs: np.ndarray, counts: np.ndarray):
    """per-graph ``(labels [n, k], probs [n, k])`` pieces, the rows outside the head's rows (label -1 in column 0) dropped: one
    compaction of the whole pass, then two slices per graph"""
    keep = labels[:, 0] >= 0
    off = np.concatenate([[0], np.cumsum(counts)])
    if not keep.all():
        off = np.concatenate([[0], np.cumsum(keep)])[off]  # the kept rows in front of every graph
        labels, probs = labels[keep], probs[keep]
    return [(labels[off[g]:off[g + 1]], probs[off[g]:off[g + 1]]) for g in range(len(counts))]


def predict_topk(model, batches: Union[Iterable, Tuple[object, Iterable]], k: int):
    """:func:`predict` with the top-k labels AND their softmax probabilities (``model.predict_topk`` per batch: eval-mode forward
    plus one launch), one device-to-host copy and one synchronisation per pass.  ``batches`` takes the forms :func:`predict` takes.

    ``(BatchStream, iterable of graph-id lists)``: one buffer for the whole pass, sized from the store's per-graph node counts
    (all labels, then all probabilities; head 0's rows, then head 1's); every batch writes its slice through ``out=``.  The result
    has one entry per graph in id order: ``(labels [n, k] int64, probs [n, k] float32)`` numpy arrays over the rows :func:`predict`
    returns for that graph (``labels[:, 0]`` is its result), or a ``(room, object)`` pair of those.  An iterable of
    batches: one entry per BATCH, the per-row arrays of ``model.predict_topk`` (``-1`` / ``0`` rows kept)."""
    from .engine import _check_k

    k = _check_k(k)
    stream, id_lists = _pass_args(model, batches, "predict_topk")
    dev = next(model.parameters()).device
    if stream is None:
        outs = [model.predict_topk(b, k) for b in batches]
        two = bool(outs) and isinstance(outs[0][0], tuple)
        flat = [t for o in outs for hd in (o if two else (o,)) for t in hd]  # labels, probs, labels, probs, ...
        if not flat:
            return []
        host = torch.cat([t.reshape(-1).view(torch.uint8) for t in flat]).cpu().numpy()  # the one copy of the pass
        sizes = np.cumsum([0] + [t.numel() * t.element_size() for t in flat])
        parts = [host[sizes[i]:sizes[i + 1]].view(np.int64 if i % 2 == 0 else np.float32).reshape(-1, k) for i in range(len(flat))]
        heads = [(parts[2 * i], parts[2 * i + 1]) for i in range(len(parts) // 2)]
        return [(heads[2 * i], heads[2 * i + 1]) for i in range(len(outs))] if two else heads
    types = _label_types(model)
    two = len(types) == 2
    all_ids = np.concatenate(id_lists) if id_lists else np.zeros(0, dtype=np.int64)
    counts = [stream.store.node_counts[t][all_ids] for t in types]
    totals = [int(c.sum()) for c in counts]
    R = sum(totals)
    buf = torch.empty(max(12 * R * k, 1), dtype=torch.uint8, device=dev)  # int64 labels [R, k], then float32 probabilities [R, k]
    labels = buf[:8 * R * k].view(torch.int64).view(R, k)
    probs = buf[8 * R * k:12 * R * k].view(torch.float32).view(R, k)
    pos = [0, totals[0]]
    for ids in id_lists:
        rows = [int(stream.store.node_counts[t][ids].sum()) for t in types]
        views = [(labels[pos[h]:pos[h] + rows[h]], probs[pos[h]:pos[h] + rows[h]]) for h in range(len(types))]
        model.predict_topk(stream.next(ids), k, out=tuple(views) if two else views[0])
        for h in range(len(types)):
            pos[h] += rows[h]
    host = buf[:12 * R * k].cpu().numpy()  # the one copy (and synchronisation) of the pass
    hl = host[:8 * R * k].view(np.int64).reshape(R, k)
    hp = host[8 * R * k:].view(np.float32).reshape(R, k)
    heads = [_split_topk(hl[:totals[0]], hp[:totals[0]], counts[0])]
    if two:
        heads.append(_split_topk(hl[totals[0]:], hp[totals[0]:], counts[1]))
        return list(zip(heads[0], heads[1]))
    return heads[0]


def _split_mc(arrays, counts: np.ndarray):
    """per-graph ``(labels [n], mean_probs [n, C], std [n], entropy [n], mutual_info [n])`` pieces, the rows outside the head's rows
    (label -1) dropped: one compaction of the whole pass, then a slice per array and graph"""
    keep = arrays[0] >= 0
    off = np.concatenate([[0], np.cumsum(counts)])
    if not keep.all():
        off = np.concatenate([[0], np.cumsum(keep)])[off]  # the kept rows in front of every graph
        arrays = [a[keep] for a in arrays]
    return [tuple(a[off[g]:off[g + 1]] for a in arrays) for g in range(len(counts))]


def predict_mc(model, batches: Union[Iterable, Tuple[object, Iterable]], samples: int, seed=None, first_step: int = 1):
    """:func:`predict` with Monte-Carlo dropout uncertainty (``model.predict_mc`` per batch: ``samples`` training-mode forwards plus
    one launch each and one finishing launch per head), one device-to-host copy and one synchronisation per pass.  ``batches`` takes
    the forms :func:`predict` takes; ``seed`` None is the model's dropout seed, and every batch draws at the steps ``first_step ..
    first_step + samples - 1``.

    ``(BatchStream, iterable of graph-id lists)``: one buffer for the whole pass, sized from the store's per-graph node counts (all
    labels, then each head's floats); every batch writes its slice through ``out=``.  The result has one entry per graph in id
    order: ``(labels [n] int64, mean_probs [n, C], std [n], entropy [n], mutual_info [n] float32)`` numpy arrays over the rows
    :func:`predict` returns for that graph, or a ``(room, object)`` pair of those.  An iterable of batches: one entry per BATCH, the
    per-row arrays of ``model.predict_mc`` (``-1`` / ``0`` rows kept)."""
    from .engine import _check_first_step, _check_samples

    samples = _check_samples(samples)
    first_step = _check_first_step(first_step, samples)
    stream, id_lists = _pass_args(model, batches, "predict_mc")
    dev = next(model.parameters()).device
    if stream is None:
        outs = [model.predict_mc(b, samples, seed, first_step) for b in batches]
        two = bool(outs) and isinstance(outs[0][0], tuple)
        flat = [t for o in outs for hd in (o if two else (o,)) for t in hd]  # labels, mean, std, entropy, mi, labels, ...
        if not flat:
            return []
        host = torch.cat([t.reshape(-1).view(torch.uint8) for t in flat]).cpu().numpy()  # the one copy of the pass
        sizes = np.cumsum([0] + [t.numel() * t.element_size() for t in flat])
        parts = [host[sizes[i]:sizes[i + 1]].view(np.int64 if i % 5 == 0 else np.float32).reshape(tuple(t.shape))
                 for i, t in enumerate(flat)]
        heads = [tuple(parts[5 * i:5 * i + 5]) for i in range(len(parts) // 5)]
        return [(heads[2 * i], heads[2 * i + 1]) for i in range(len(outs))] if two else heads
    types = _label_types(model)
    two = len(types) == 2
    classes = model.native().head_classes()
    all_ids = np.concatenate(id_lists) if id_lists else np.zeros(0, dtype=np.int64)
    counts = [stream.store.node_counts[t][all_ids] for t in types]
    totals = [int(c.sum()) for c in counts]
    nbytes = 8 * sum(totals) + 4 * sum(r * (c + 3) for r, c in zip(totals, classes))
    buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)  # every head's int64 labels, then each head's float32 arrays

    def carve(b, view):
        """per head (labels [R], mean [R, C], std [R], entropy [R], mi [R]) inside the pass buffer `b`"""
        heads, lo, fo = [], 0, 8 * sum(totals)
        for r, c in zip(totals, classes):
            lab = view(b[lo:lo + 8 * r], False)
            fl = view(b[fo:fo + 4 * r * (c + 3)], True)
            lo, fo = lo + 8 * r, fo + 4 * r * (c + 3)
            heads.append((lab, fl[:r * c].reshape(r, c), fl[r * c:r * c + r], fl[r * c + r:r * c + 2 * r], fl[r * c + 2 * r:]))
        return heads

    dev_heads = carve(buf, lambda b, f32: b.view(torch.float32 if f32 else torch.int64))
    pos = [0, 0]
    for ids in id_lists:
        rows = [int(stream.store.node_counts[t][ids].sum()) for t in types]
        views = [tuple(a[pos[h]:pos[h] + rows[h]] for a in dev_heads[h]) for h in range(len(types))]
        model.predict_mc(stream.next(ids), samples, seed, first_step, out=tuple(views) if two else views[0])
        for h in range(len(types)):
            pos[h] += rows[h]
    host = buf[:nbytes].cpu().numpy()  # the one copy (and synchronisation) of the pass
    host_heads = carve(host, lambda b, f32: b.view(np.float32 if f32 else np.int64))
    heads = [_split_mc(list(hd), c) for hd, c in zip(host_heads, counts)]
    return list(zip(heads[0], heads[1])) if two else heads[0]


def saliency(model, batches: Union[Iterable, Tuple[object, Iterable]], groups=((0, 3), (3, 6), (6, None)), **kw):
    """Gradient saliency over ``batches`` with ONE device-to-host copy at the end of the pass (``model.saliency`` per batch: eval-mode
    forward, one seed launch, the input-gradient chain and one reduction launch per node type; nothing synchronises in between).
    ``batches`` takes the forms :func:`predict` takes; ``groups`` and ``**kw`` (``target``, ``wrt``, ``head``) go to
    ``model.saliency``.  Every batch explains all its output rows together: the gradient of the sum of each row's own
    predicted-class logit.

    ``(BatchStream, iterable of graph-id lists)``: one entry per graph in id order, ``{node_type: (gxi [n], gnorm [n], groups [n,
    n_groups])}`` of numpy float32 arrays over the graph's rows of that node type (homogeneous models: the one triple).  An
    iterable of batches: one entry per BATCH in that structure."""
    stream, id_lists = _pass_args(model, batches, "saliency")
    per_batch = [model.saliency(stream.next(ids) if stream is not None else b, groups=groups, **kw)
                 for ids, b in (zip(id_lists, id_lists) if stream is not None else ((None, b) for b in batches))]
    if not per_batch:
        return []
    homog = isinstance(per_batch[0], tuple)
    dicts = [{None: r} if homog else r for r in per_batch]
    flat = [t.reshape(-1) for d in dicts for trip in d.values() for t in trip]
    host = torch.cat(flat).cpu().numpy() if flat else np.zeros(0, dtype=np.float32)  # the one copy (and synchronisation) of the pass
    pos = 0
    out = []
    for bi, d in enumerate(dicts):
        arrays = {}
        for t, trip in d.items():
            parts = []
            for v in trip:
                parts.append(host[pos:pos + v.numel()].reshape(tuple(v.shape)))
                pos += v.numel()
            arrays[t] = tuple(parts)
        if stream is None:
            out.append(arrays[None] if homog else arrays)
            continue
        ids = id_lists[bi]
        node_types = stream.store.node_types
        offs = {t: np.concatenate([[0], np.cumsum(stream.store.node_counts[t if t is not None else node_types[0]][ids])]) for t in arrays}
        for g in range(len(ids)):
            piece = {t: tuple(a[offs[t][g]:offs[t][g + 1]] for a in trip) for t, trip in arrays.items()}
            out.append(piece[None] if homog else piece)
    return out
