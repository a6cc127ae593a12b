"""Plain-torch CPU references of the readout tails (csrc/semisup.hip) and the two linear heads (csrc/heads.hip): no project code.

    y = keep * act(z) / (1 - p)            over the first `classes` (or F) columns
    tail:   rows = y, or with a pool the segment mean of y over each pooled row's leaves (divisor max(deg, 1), empty row = 0);
            SUM cross entropy over the rows with  mask & label != ignored & 0 <= label < classes
    heads:  logits_h = y W_h^T + b_h on the rows of head h; the same CE per head, summed

Every function evaluates in `dtype`: float64 is the reference, float32 (the same formulas, torch's own association) is the
yardstick a float32 kernel is measured against (yardstick / within below).  tests/test_tail_reference.py checks this file
against torch.nn.functional on the CPU."""
import numpy as np
import torch
import torch.nn.functional as F

ACT_NONE, ACT_RELU, ACT_ELU = 0, 1, 2


def _act(z, act):
    if act == ACT_RELU:
        return torch.relu(z)
    if act == ACT_ELU:
        return F.elu(z)
    assert act == ACT_NONE
    return z


def _y(z, width, act, keep, p, dtype):
    """(leaf z [n, width] with requires_grad, y) in dtype"""
    zl = z[:, :width].detach().to("cpu", dtype).clone().requires_grad_(True)
    y = _act(zl, act)
    if p > 0:
        y = y * keep[:, :width].to("cpu", dtype) / (1.0 - p)
    return zl, y


def _masked_ce(logits, labels, valid):
    """per-row CE where valid (0 elsewhere); labels of invalid rows are never used as an index"""
    lab = torch.where(valid, labels, torch.zeros_like(labels))
    lse = torch.logsumexp(logits, dim=1)
    return torch.where(valid, lse - logits.gather(1, lab[:, None])[:, 0], torch.zeros_like(lse))


def _top2_gap(logits):
    if logits.shape[1] < 2:
        return torch.full((logits.shape[0],), float("inf"), dtype=logits.dtype)
    t = torch.topk(logits, 2, dim=1).values
    return t[:, 0] - t[:, 1]


def _first_argmax(logits):
    """index of the first maximum of every row (spelled out: the rule must not depend on a library's tie-breaking)"""
    m = logits.max(dim=1, keepdim=True).values
    idx = torch.arange(logits.shape[1])[None, :].expand_as(logits)
    return torch.where(logits == m, idx, torch.full_like(idx, logits.shape[1])).min(dim=1).values


def pool_csr_csc(n_pool, n_leaves, edges):
    """CSR by pooled row and CSC by leaf of the pool edges [(leaf, pooled row), ...], both stable in edge order (the order a
    stable sort of the edge list by destination / by source produces).  Returns int32 numpy (rowptr, col, t_rowptr, t_col)."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    leaf, row = e[:, 0], e[:, 1]
    o = np.argsort(row, kind="stable")
    rowptr = np.zeros(n_pool + 1, dtype=np.int64)
    np.add.at(rowptr, row + 1, 1)
    t = np.argsort(leaf, kind="stable")
    t_rowptr = np.zeros(n_leaves + 1, dtype=np.int64)
    np.add.at(t_rowptr, leaf + 1, 1)
    return (np.cumsum(rowptr).astype(np.int32), leaf[o].astype(np.int32), np.cumsum(t_rowptr).astype(np.int32), row[t].astype(np.int32))


def tail_reference(z, classes, act, keep, p, labels, mask, ignored, pool=None, dtype=torch.float64):
    """z [n_rows, >= classes]; keep [n_rows, >= classes] (ignored when p == 0); labels int64 and mask (bool / uint8 or None) per
    CE row; pool = (rowptr, col) CSR by pooled row over the leaf rows of z, or None.  Returns a dict:
    loss (SUM), row_loss, row_valid, bad (rows with a counted label outside [0, classes)), dz [n_rows, classes], pred (first-maximum
    argmax per CE row), gap (top-two gap per CE row), correct, total (over the rows of mask: pred == label)."""
    zl, y = _y(z, classes, act, keep, p, dtype)
    if pool is not None:
        rowptr = torch.as_tensor(np.asarray(pool[0]), dtype=torch.int64)
        col = torch.as_tensor(np.asarray(pool[1]), dtype=torch.int64)
        n_pool = rowptr.numel() - 1
        deg = rowptr[1:] - rowptr[:-1]
        seg = torch.repeat_interleave(torch.arange(n_pool), deg)
        rows = torch.zeros(n_pool, classes, dtype=dtype).index_add(0, seg, y[col]) / deg.clamp(min=1).to(dtype)[:, None]
    else:
        rows = y
    n = rows.shape[0]
    labels = torch.as_tensor(labels).to("cpu", torch.int64)
    m = torch.ones(n, dtype=torch.bool) if mask is None else torch.as_tensor(mask).to("cpu") != 0
    counted = m & (labels != ignored)
    valid = counted & (labels >= 0) & (labels < classes)
    row_loss = _masked_ce(rows, labels, valid)
    loss = row_loss.sum()
    if zl.numel():
        loss.backward()
    pred = _first_argmax(rows.detach()) if n else torch.zeros(0, dtype=torch.int64)
    return {
        "loss": loss.detach(), "row_loss": row_loss.detach(), "row_valid": valid.to(dtype), "bad": int((counted & ~valid).sum()),
        "dz": zl.grad if zl.grad is not None else torch.zeros_like(zl), "pred": pred, "gap": _top2_gap(rows.detach()),
        "correct": int((m & (pred == labels)).sum()), "total": int(m.sum()),
    }


def head_members(n, member0, member1):
    """head_member's rules: member[0] None = every row; member[1] None = the complement of member[0] (empty when both are None)"""
    m0 = torch.ones(n, dtype=torch.bool) if member0 is None else torch.as_tensor(member0).to("cpu") != 0
    if member1 is not None:
        m1 = torch.as_tensor(member1).to("cpu") != 0
    elif member0 is not None:
        m1 = ~m0
    else:
        m1 = torch.zeros(n, dtype=torch.bool)
    return m0, m1


def linear_heads_reference(z, Fw, W0, b0, W1, b1, act, keep, p, labels, mask, member0, member1, ignored, dtype=torch.float64):
    """Returns a dict: loss, row_loss (loss_0 + loss_1), row_valid (valid_0 + valid_1), bad, dz [n_rows, F], dW [2], db [2],
    correct [2], total [2] (over member_h & mask: first-maximum argmax == label), gap [2] (top-two gap per row and head),
    counted [2] (member_h & mask)."""
    zl, y = _y(z, Fw, act, keep, p, dtype)
    n = zl.shape[0]
    labels = torch.as_tensor(labels).to("cpu", torch.int64)
    m = torch.ones(n, dtype=torch.bool) if mask is None else torch.as_tensor(mask).to("cpu") != 0
    members = head_members(n, member0, member1)
    Ws = [w.detach().to("cpu", dtype).clone().requires_grad_(True) for w in (W0, W1)]
    bs = [b.detach().to("cpu", dtype).clone().requires_grad_(True) for b in (b0, b1)]
    out = {"correct": [], "total": [], "gap": [], "counted": [], "bad": 0}
    row_loss = torch.zeros(n, dtype=dtype)
    row_valid = torch.zeros(n, dtype=dtype)
    for h in range(2):
        C = Ws[h].shape[0]
        logits = y @ Ws[h].t() + bs[h]
        counted = members[h] & m
        live = counted & (labels != ignored)
        valid = live & (labels >= 0) & (labels < C)
        row_loss = row_loss + _masked_ce(logits, labels, valid)
        row_valid = row_valid + valid.to(dtype)
        out["bad"] += int((live & ~valid).sum())
        pred = _first_argmax(logits.detach())
        out["correct"].append(int((counted & (pred == labels)).sum()))
        out["total"].append(int(counted.sum()))
        out["gap"].append(_top2_gap(logits.detach()))
        out["counted"].append(counted)
    loss = row_loss.sum()
    loss.backward()
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)  # noqa: E731
    out.update(loss=loss.detach(), row_loss=row_loss.detach(), row_valid=row_valid, dz=zero(zl), dW=[zero(w) for w in Ws],
               db=[zero(b) for b in bs])
    return out


# ---- the float32 yardstick -------------------------------------------------------------------------------------------------------
REL_FLOOR = 1e-6  # relative errors are measured over elements with |ref| above this
F32_EPS = 2.0 ** -23


def yardstick(f32, ref):
    """(max abs error, max relative error over |ref| > 1e-6) of a float32 evaluation against the float64 reference"""
    ref = ref.double().reshape(-1)
    err = (f32.double().reshape(-1) - ref).abs()
    if err.numel() == 0:
        return 0.0, 0.0
    big = ref.abs() > REL_FLOOR
    rel = float((err[big] / ref[big].abs()).max()) if bool(big.any()) else 0.0
    return float(err.max()), rel


def within(got, ref, yard, factor=4.0, signed_sum=False):
    """A float32 kernel's result against the reference.  An element passes when its error is within the floor of 4 float32 ulps of
    the largest |ref| of the tensor, or within BOTH `factor` x the yardstick's max abs error and (where |ref| > 1e-6) `factor` x its
    max relative error: the kernel's association differs from torch's (a butterfly over 16 lanes, fmaf chains) and its expf / logf /
    expm1f are a few ulp from the host's.

    signed_sum: the tensor is a matrix product of signed terms (the linear heads' dz, dW, db).  The float32 error of sum_i a_i b_i
    is bounded by n eps sum_i |a_i b_i| plus the propagated error of the a_i -- a quantity of the TERMS, not of the result -- so an
    element that nearly cancels has no bounded relative error in any float32 evaluation, and the maximum of err / |ref| over the
    tensor is decided by which evaluation happens to be lucky on the few smallest elements (dW of 64 + 64 classes at F = 1024: the
    kernel's max abs error is 1.25 x the yardstick's, its max relative error, on one element of 131072 with |ref| ~ 1e-4, 10 x).
    Such a tensor is held to `factor` x the max abs error alone.  Returns (ok, message with the measured figures)."""
    ref = ref.double().reshape(-1)
    got = got.double().reshape(-1)
    if ref.numel() == 0:
        return True, "empty"
    err = (got - ref).abs()
    floor = 4.0 * F32_EPS * float(ref.abs().max())
    big = ref.abs() > REL_FLOOR
    rel = torch.where(big, err / ref.abs().clamp(min=REL_FLOOR), torch.zeros_like(err))
    ok = err <= factor * yard[0]
    if not signed_sum:
        ok &= rel <= factor * yard[1]
    ok |= err <= floor
    ok &= ~torch.isnan(got)
    msg = (f"max abs err {float(err.max()):.3e} (yardstick {yard[0]:.3e}, floor {floor:.3e}), max rel err {float(rel.max()):.3e} "
           f"(yardstick {yard[1]:.3e}{', not charged: signed sum' if signed_sum else ''}), {int((~ok).sum())} of {ok.numel()} "
           "elements outside")
    return bool(ok.all()), msg
