"""Float64 numpy / torch restatements of the gradient-saliency kernels and of the executor's input-gradient path.

``seed_reference``         the output gradient selecting what is explained (hmp_saliency_seed)
``selected_rows``          the three row-selection modes
``scores_reference``       gradient x input, gradient norm and per-range sums per row (hmp_saliency_scores)
``top_from_scores``        the k sources with the largest |score| per destination row (hmp_saliency_topk): an exact function of the
                           float32 score array -- it only compares and copies -- so results are compared bit for bit
``oracle_input_gradients`` the ``oracle.models`` twin in float64 on ``x.double().requires_grad_()``: sum of the selected logits or
                           log-probabilities, ``.backward()``, and the smallest |pre-activation| over all ReLU inputs of the run
"""
import copy
from unittest import mock

import numpy as np
import torch

SEL_ALL, SEL_MASK, SEL_ORDINAL = 0, 1, 2
WRT_LOGIT, WRT_LOGPROB = 0, 1


def selected_rows(n_rows, mode=SEL_ALL, mask=None, p=0, ptr=None):
    """bool [n_rows]: ALL; MASK: mask != 0; ORDINAL: row ptr[g] + p of every graph g with more than p rows"""
    if mode == SEL_ALL:
        return np.ones(n_rows, dtype=bool)
    if mode == SEL_MASK:
        return np.asarray(mask).astype(bool).copy()
    sel = np.zeros(n_rows, dtype=bool)
    ptr = np.asarray(ptr, dtype=np.int64)
    for g in range(len(ptr) - 1):
        if ptr[g + 1] - ptr[g] > p and ptr[g] + p < n_rows:
            sel[ptr[g] + p] = True
    return sel


def first_argmax(z):
    """first maximum per row (torch.argmax / np.argmax on finite values), 0 for a row without columns"""
    z = np.asarray(z)
    return np.argmax(z, axis=1).astype(np.int64) if z.shape[1] else np.zeros(z.shape[0], dtype=np.int64)


def seed_reference(z, n_classes, ld_g, target=None, sel=None, wrt=WRT_LOGIT):
    """float64 [n_rows, ld_g]: onehot(c) or onehot(c) - softmax(z) on the selected rows, 0 elsewhere and in columns >= n_classes;
    c = target where given and in [0, n_classes), else the first-maximum argmax of the float32 logits"""
    z = np.asarray(z)[:, :n_classes]
    n = z.shape[0]
    cls = first_argmax(z)
    if target is not None:
        t = np.asarray(target, dtype=np.int64)
        ok = (t >= 0) & (t < n_classes)
        cls = np.where(ok, t, cls)
    out = np.zeros((n, ld_g), dtype=np.float64)
    sel = np.ones(n, dtype=bool) if sel is None else np.asarray(sel, dtype=bool)
    z64 = z.astype(np.float64)
    for r in np.nonzero(sel)[0]:
        out[r, cls[r]] = 1.0
        if wrt == WRT_LOGPROB:
            e = np.exp(z64[r] - z64[r].max())
            out[r, :n_classes] -= e / e.sum()
    return out, cls


def scores_reference(g, x, F, groups=()):
    """float64 (gxi [n], gnorm [n], groups [n, n_groups], sum |g x| [n]) over the first F columns; ranges clipped to [0, F)"""
    g = np.asarray(g, dtype=np.float64)[:, :F]
    x = np.asarray(x, dtype=np.float64)[:, :F]
    p = g * x
    cols = []
    for lo, hi in groups:
        lo, hi = max(0, int(lo)), min(F, F if hi is None else int(hi))
        cols.append(p[:, lo:hi].sum(axis=1) if hi > lo else np.zeros(p.shape[0]))
    grp = np.stack(cols, axis=1) if cols else np.zeros((p.shape[0], 0))
    return p.sum(axis=1), np.sqrt((g * g).sum(axis=1)), grp, np.abs(p).sum(axis=1)


def top_from_scores(score, ei, n_src, n_dst, k, sel=None, prefill=(-7, np.float32(-7.0))):
    """(src int64 [n_dst, k], score float32 [n_dst, k]): per selected destination row the k distinct sources of its in-range edges
    with the largest |score|, descending, equal magnitudes by ascending source; the signed float32 score; -1 / 0 past the row's
    sources.  Rows outside ``sel`` keep ``prefill``."""
    score = np.asarray(score, dtype=np.float32)
    ei = np.asarray(ei, dtype=np.int64).reshape(2, -1)
    src = np.full((n_dst, k), prefill[0], dtype=np.int64)
    out = np.full((n_dst, k), prefill[1], dtype=np.float32)
    ok = (ei[0] >= 0) & (ei[0] < n_src) & (ei[1] >= 0) & (ei[1] < n_dst)
    sel = np.ones(n_dst, dtype=bool) if sel is None else np.asarray(sel, dtype=bool)
    for d in range(n_dst):
        if not sel[d]:
            continue
        cand = sorted(set(ei[0][ok & (ei[1] == d)].tolist()), key=lambda j: (-abs(float(score[j])), j))[:k]
        src[d] = -1
        out[d] = 0.0
        for c, j in enumerate(cand):
            src[d, c] = j
            out[d, c] = score[j]
    return src, out


def _double_inputs(batch):
    """the batch on the CPU with float64 features; returns (batch, {key: leaf x that requires grad}); key None: homogeneous"""
    b = batch.to("cpu")
    leaves = {}
    if hasattr(b, "node_types"):
        for t in b.node_types:
            if "x" in b[t]:
                b[t].x = b[t].x.double().requires_grad_()
                leaves[t] = b[t].x
        for et in b.edge_types:
            if "edge_attr" in b[et]:
                b[et].edge_attr = b[et].edge_attr.double()
    else:
        b.x = b.x.double().requires_grad_()
        leaves[None] = b.x
        if getattr(b, "edge_attr", None) is not None:
            b.edge_attr = b.edge_attr.double()
    return b, leaves


def oracle_input_gradients(ora, batch, target=None, rows=None, wrt="logit", head=None, train=False):
    """({node type | None: d s / d x float64}, smallest |ReLU input| of the run or inf, the head's logits float64)

    ``s`` = sum over ``rows`` (bool over the head's output rows; None: all) of the logit (``wrt="logit"``) or log-probability
    (``"logprob"``) of ``target[row]`` (int64; None: the row's own argmax).  ``head``: index into a two-headed oracle's outputs."""
    o64 = copy.deepcopy(ora).double()
    o64.train(train)
    b, leaves = _double_inputs(batch)
    import torch.nn.functional as F

    smallest = [float("inf")]
    real_relu = F.relu

    def relu(x, *a, **k):
        if x.numel():
            smallest[0] = min(smallest[0], float(x.detach().abs().min()))
        return real_relu(x, *a, **k)

    with mock.patch.object(F, "relu", relu):
        out = o64(b)
    if head is not None:
        out = out[head]
    n = out.size(0)
    cls = out.detach().argmax(dim=1) if target is None else torch.as_tensor(target, dtype=torch.int64)
    val = out if wrt == "logit" else torch.log_softmax(out, dim=1)
    picked = val[torch.arange(n), cls]
    if rows is not None:
        picked = picked[torch.as_tensor(rows, dtype=torch.bool)]
    picked.sum().backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in leaves.items()}
    return grads, smallest[0], out.detach()
