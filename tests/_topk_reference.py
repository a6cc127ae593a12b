"""Plain-torch CPU reference of the top-k launches (csrc/tail_fns.h topk_group): no project code.  It sits on tests/_tail_reference.py.

    scores   per net kind, the formulas of tail_reference / linear_heads_reference in `dtype`:
               tail:   y = act(z), or with a pool the segment mean of y over each pooled row's leaves (empty row = 0)
               heads:  logits_h = y W_h^T + b_h
    order    a stable descending sort: scores descending, equal scores by ascending class (+0.0 == -0.0)
    probs    the float64 softmax

float64 is the reference; the same formulas in float32 are the yardstick whose distance to float64 (`yard`, the largest absolute
score difference of a case) sizes the two tolerances below.

    probabilities   |probs[r, j] - p64[r, labels[r, j]]| <= 1e-5 + yard / 2 on every written element.  1e-5 is the project's
                    standing fp32 bound; a softmax entry moves by at most 1/4 of a score's error, taken twice for slack.
    order           exact where the kernel reads the values the reference reads (yard == 0, or a monotone activation of them).
                    Else a row is left out of the ORDER check when any adjacent float64 gap among its top k + 1 scores is
                    non-zero and at most 64 x yard (an exact tie is built from equal operands and still compared); at most 1 %
                    of a case's rows, asserted by order_rows() on the reference alone, before anything is launched."""
import numpy as np
import torch

from _tail_reference import _y

TOPK_MAX = 8
P_TOL = 1e-5


def tail_scores(z, classes, act, pool=None, dtype=torch.float64):
    """[rows, classes]: act(z), or with pool = (rowptr, col) the segment mean over each pooled row's leaves (tail_reference's lines)"""
    _, y = _y(z, classes, act, None, 0.0, dtype)
    y = y.detach()
    if pool is None:
        return y
    rowptr = torch.as_tensor(np.asarray(pool[0]), dtype=torch.int64)
    col = torch.as_tensor(np.asarray(pool[1]), dtype=torch.int64)
    n_pool = rowptr.numel() - 1
    deg = rowptr[1:] - rowptr[:-1]
    seg = torch.repeat_interleave(torch.arange(n_pool), deg)
    return torch.zeros(n_pool, classes, dtype=dtype).index_add(0, seg, y[col]) / deg.clamp(min=1).to(dtype)[:, None]


def head_scores(z, F, Ws, bs, act, dtype=torch.float64):
    """both heads' logits [rows, classes_h] (linear_heads_reference's line)"""
    _, y = _y(z, F, act, None, 0.0, dtype)
    return [(y @ w.to(dtype).t() + b.to(dtype)).detach() for w, b in zip(Ws, bs)]


def yard_of(s32, s64):
    """largest |float32 yardstick - float64| score entry"""
    return float((s32.double() - s64).abs().max()) if s64.numel() else 0.0


def stable_order(scores):
    """class indices [rows, classes] in the total order: descending score, equal scores by ascending class"""
    return torch.sort(scores, dim=1, descending=True, stable=True).indices


def order_rows(s64, k, yard, tag):
    """bool [rows]: the rows whose order is compared.  yard == 0: all.  The 1 % cap is asserted here, on the reference alone."""
    n = s64.shape[0]
    if yard == 0.0 or n == 0 or s64.shape[1] < 2:
        return torch.ones(n, dtype=torch.bool)
    top = torch.sort(s64, dim=1, descending=True).values[:, :k + 1]
    gap = top[:, :-1] - top[:, 1:]
    skip = ((gap > 0) & (gap <= 64.0 * yard)).any(dim=1)
    assert int(skip.sum()) * 100 <= n, f"{tag}: {int(skip.sum())} of {n} rows have a top-{k + 1} gap inside {64.0 * yard:.3e}"
    return ~skip


def check_topk(labels, probs, s64, k, yard, use, tag, members=None):
    """labels [rows, k] int64 and probs [rows, k] float32 (host) of a launch against the float64 scores s64 [rows, C]; either may be
    None (that output was skipped).  members: bool [rows], rows outside hold -1 / 0 in all k columns.  use: order_rows()'s rows."""
    n, C = s64.shape
    kk = min(k, C)
    mem = torch.ones(n, dtype=torch.bool) if members is None else members
    if labels is not None:
        assert labels.dtype == torch.int64 and tuple(labels.shape) == (n, k), tag
        assert bool((labels[~mem] == -1).all()), f"{tag}: a row outside the head holds a label"
        assert bool((labels[mem][:, kk:] == -1).all()), f"{tag}: a column past the {C} classes holds a label"
        top = labels[mem][:, :kk]
        assert bool(((top >= 0) & (top < C)).all()), f"{tag}: a label outside [0, {C})"
        srt = torch.sort(top, dim=1).values
        assert bool((srt[:, 1:] != srt[:, :-1]).all()), f"{tag}: a row names a class twice"
        want = stable_order(s64)[:, :kk]
        on = mem & use
        bad = (labels[on][:, :kk] != want[on]).any(dim=1)
        assert not bool(bad.any()), (f"{tag}: order differs on {int(bad.sum())} rows, first: got "
                                     f"{labels[on][bad][0].tolist()} want {want[on][bad][0].tolist()}")
    if probs is not None:
        assert probs.dtype == torch.float32 and tuple(probs.shape) == (n, k), tag
        assert bool((probs[~mem] == 0).all()), f"{tag}: a row outside the head holds a probability"
        assert bool((probs[mem][:, kk:] == 0).all()), f"{tag}: a column past the {C} classes holds a probability"
    if labels is None or probs is None or not bool(mem.any()):
        return
    p64 = torch.softmax(s64[mem], dim=1)
    want_p = p64.gather(1, labels[mem][:, :kk])
    err = (probs[mem][:, :kk].double() - want_p).abs()
    tol = P_TOL + 0.5 * yard
    print(f"{tag}: max |p - p64| {float(err.max()):.3e} (tolerance {tol:.3e}, yard {yard:.3e})")
    assert float(err.max()) <= tol, f"{tag}: probability off by {float(err.max()):.3e} > {tol:.3e}"
    if k == C and C <= TOPK_MAX:
        tot = probs[mem].double().sum(dim=1)
        assert float((tot - 1.0).abs().max()) <= P_TOL * C, f"{tag}: probabilities of a full row sum to {tot.tolist()[:4]}"
