"""Differentiable operators over the op-level C ABI (``include/hydra_mp.h`` sections 1-5 and 9).

The SAGE / GAT families run as ONE native program per step (:mod:`hydra_gnn_amd.engine`).  The homogeneous GCN / GIN
family of the reference's Stanford3DSG configurations (``models/utils.py:15-26``, ``models/homogeneous_network.py:93-97``;
SURVEY.md 8(f) row 2) works on graphs of 2..27 nodes and is composed here op by op: every function below is a
``torch.autograd.Function`` whose forward and backward are calls into ``libhydra_mp.so`` -- torch provides tensors, the
stream and the autograd tape only.  There is no CPU path: CPU tensors raise.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib


def _dev(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise _lib.HydraMPError(f"{what} is on the CPU; hydra_gnn_amd has no CPU fallback")
    if t.dtype != torch.float32:
        raise _lib.HydraMPError(f"{what}: the native operators compute in fp32 (got {t.dtype})")


def _rows(t: torch.Tensor) -> torch.Tensor:
    """row-major with unit column stride (the kernels take a leading dimension)"""
    return t if (t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.size(1)) else t.contiguous()


class GraphPlan:
    """CSR (by destination) + CSC lists of one square ``edge_index`` (``hmp_plan_build``), built once per batch and
    shared by every layer; ``dinv`` is GCN's ``deg^-1/2`` with the replaced self loops counted (``hmp_gcn_norm``)."""

    def __init__(self, edge_index: torch.Tensor, num_nodes: int, num_src: Optional[int] = None):
        """``num_src``: rows of the source side when the edge type is bipartite (LeafPool over ``room -> room_virtual``);
        the GCN / GIN operators need the square form"""
        if not edge_index.is_cuda:
            raise _lib.HydraMPError("edge_index is on the CPU; hydra_gnn_amd has no CPU fallback")
        lib = _lib.require_device()
        ei = edge_index.to(torch.int64).contiguous()
        E, d, n = int(ei.size(1)), ei.device, int(num_nodes)
        ns = n if num_src is None else int(num_src)
        self.n, self.n_src, self.E, self.device = n, ns, E, d
        i32 = lambda k: torch.empty(max(k, 1), dtype=torch.int32, device=d)
        self._t = [i32(n + 1), i32(E), i32(E), i32(ns + 1), i32(E), i32(E)]
        self.plan = _lib.Plan(ns, n, E, *[t.data_ptr() for t in self._t])
        scratch = torch.empty(max(int(lib.hmp_plan_scratch_bytes(E, ns, n)), 16), dtype=torch.uint8, device=d)
        self.status = torch.zeros(1, dtype=torch.int32, device=d)
        with torch.cuda.device(d):
            _lib.check(lib.hmp_plan_build(ei.data_ptr() if E > 0 else None, self.plan, scratch.data_ptr(), self.status.data_ptr(),
                                          _lib.stream_ptr()))
        self._ei, self._scratch = ei, scratch  # alive until the stream has consumed them
        self._dinv: Optional[torch.Tensor] = None

    @property
    def dinv(self) -> torch.Tensor:
        if self._dinv is None:
            self._dinv = torch.empty(max(self.n, 1), dtype=torch.float32, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(_lib.load().hmp_gcn_norm(self.plan, self._dinv.data_ptr(), _lib.stream_ptr()))
        return self._dinv


def _gemm(a, trans_a, b, trans_b, M, N, K) -> torch.Tensor:
    c = torch.empty((M, N), dtype=torch.float32, device=a.device)
    if M == 0 or N == 0:
        return c
    if K == 0:
        return c.zero_()
    with torch.cuda.device(a.device):
        _lib.check(_lib.load().hmp_gemm_f32(a.data_ptr(), a.stride(0), trans_a, b.data_ptr(), b.stride(0), trans_b, c.data_ptr(),
                                            c.stride(0), M, N, K, _lib.stream_ptr()))
    return c


def _colsum(g: torch.Tensor) -> torch.Tensor:
    out = torch.empty(g.size(1), dtype=torch.float32, device=g.device)
    with torch.cuda.device(g.device):
        _lib.check(_lib.load().hmp_colsum(g.data_ptr(), g.stride(0), g.size(0), g.size(1), out.data_ptr(), _lib.stream_ptr()))
    return out


class _Project(torch.autograd.Function):
    """``x @ weight.T`` (nn.Linear layout) on the fp32 matrix pipe; no bias (biases ride in :func:`bias_act_drop`)."""

    @staticmethod
    def forward(ctx, x, weight):
        _lib.require_device()
        _dev(x, "x"), _dev(weight, "weight")
        x, weight = _rows(x), _rows(weight)
        ctx.save_for_backward(x, weight)
        return _gemm(x, 0, weight, 1, x.size(0), weight.size(0), x.size(1))

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        g = _rows(g)
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = _gemm(g, 0, weight, 0, g.size(0), weight.size(1), weight.size(0))
        if ctx.needs_input_grad[1]:
            gw = _gemm(g, 1, x, 0, weight.size(0), weight.size(1), g.size(0))
        return gx, gw


class _WSum(torch.autograd.Function):
    """``hmp_segment_wsum``: GCN's symmetric-normalised sum (``w = plan.dinv``) or GIN's ``sum + (1 + eps) * self``."""

    @staticmethod
    def forward(ctx, z, plan: GraphPlan, gcn: bool, eps):
        _dev(z, "z")
        z = _rows(z)
        if z.size(0) != plan.n or plan.n_src != plan.n:
            raise _lib.HydraMPError(f"segment_wsum: {z.size(0)} rows for a plan over {plan.n_src} -> {plan.n} nodes (square plans only)")
        ctx.plan, ctx.gcn = plan, gcn
        ctx.save_for_backward(z, eps if eps is not None else z.new_empty(0))
        ctx.has_eps = eps is not None
        return _WSum._run(z, plan, gcn, eps, 0)

    @staticmethod
    def _run(z, plan, gcn, eps, transpose):
        out = torch.empty((z.size(0), z.size(1)), dtype=torch.float32, device=z.device)
        if z.numel() == 0:
            return out
        w = plan.dinv.data_ptr() if gcn else None
        with torch.cuda.device(z.device):
            _lib.check(_lib.load().hmp_segment_wsum(z.data_ptr(), z.stride(0), z.size(1), plan.plan, transpose, w,
                                                    eps.data_ptr() if eps is not None else None, out.data_ptr(), out.stride(0),
                                                    _lib.stream_ptr()))
        return out

    @staticmethod
    def backward(ctx, g):
        z, eps = ctx.saved_tensors
        eps = eps if ctx.has_eps else None
        g = _rows(g)
        gz = _WSum._run(g, ctx.plan, ctx.gcn, eps, 1) if ctx.needs_input_grad[0] else None
        geps = None
        if ctx.has_eps and ctx.needs_input_grad[3]:
            geps = torch.empty_like(eps)
            if z.numel() == 0:
                geps.zero_()
            else:
                with torch.cuda.device(z.device):
                    _lib.check(_lib.load().hmp_rowdot_sum(g.data_ptr(), g.stride(0), z.data_ptr(), z.stride(0), z.size(0), z.size(1),
                                                          geps.data_ptr(), _lib.stream_ptr()))
        return gz, None, None, geps


class _BiasActDrop(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, act: int, p: float, seed: int, rng_step: int, rng_stream: int):
        _dev(x, "x")
        x = _rows(x)
        y = torch.empty((x.size(0), x.size(1)), dtype=torch.float32, device=x.device)
        if x.numel():
            with torch.cuda.device(x.device):
                _lib.check(_lib.load().hmp_bias_act_drop_fwd(x.data_ptr(), x.stride(0), x.size(0), x.size(1),
                                                             bias.data_ptr() if bias is not None else None, int(act), float(p), seed,
                                                             rng_step, rng_stream, y.data_ptr(), y.stride(0), _lib.stream_ptr()))
        ctx.act, ctx.p, ctx.has_bias = int(act), float(p), bias is not None
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        g = _rows(g)
        if ctx.act != _lib.ACT_NONE:
            gx = torch.empty_like(y)
            if y.numel():
                with torch.cuda.device(y.device):
                    _lib.check(_lib.load().hmp_bias_act_drop_bwd(g.data_ptr(), g.stride(0), y.data_ptr(), y.stride(0), y.size(0), y.size(1),
                                                                 ctx.act, ctx.p, gx.data_ptr(), gx.stride(0), _lib.stream_ptr()))
        else:
            gx = g
        gb = _colsum(gx) if ctx.has_bias and ctx.needs_input_grad[1] else None
        return gx, gb, None, None, None, None, None


class _BatchNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum: float, eps: float, training: bool):
        _dev(x, "x")
        x = _rows(x)
        n, F = x.shape
        y = torch.empty((n, F), dtype=torch.float32, device=x.device)
        save = torch.empty((2, F), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().hmp_batchnorm_fwd(x.data_ptr(), x.stride(0), n, F, gamma.data_ptr(), beta.data_ptr(),
                                                     running_mean.data_ptr(), running_var.data_ptr(), float(momentum), float(eps),
                                                     int(training), y.data_ptr(), y.stride(0), save.data_ptr(), _lib.stream_ptr()))
        ctx.training = training
        ctx.save_for_backward(x, gamma, save)
        ctx.mark_non_differentiable(running_mean, running_var)
        return y

    @staticmethod
    def backward(ctx, g):
        x, gamma, save = ctx.saved_tensors
        g = _rows(g)
        n, F = x.shape
        gx = torch.empty_like(x)
        gg, gb = torch.empty_like(gamma), torch.empty_like(gamma)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().hmp_batchnorm_bwd(g.data_ptr(), g.stride(0), x.data_ptr(), x.stride(0), n, F, gamma.data_ptr(),
                                                     save.data_ptr(), int(ctx.training), gx.data_ptr(), gx.stride(0), gg.data_ptr(),
                                                     gb.data_ptr(), _lib.stream_ptr()))
        return gx, gg, gb, None, None, None, None, None


class _SegmentMean(torch.autograd.Function):
    """``hmp_segment_mean_fwd`` / ``_bwd``: mean of the source rows over the incoming edges (LeafPool; zeros for rows
    without an edge)."""

    @staticmethod
    def forward(ctx, x, plan: GraphPlan):
        _dev(x, "x")
        x = _rows(x)
        if x.size(0) != plan.n_src:
            raise _lib.HydraMPError(f"segment_mean: {x.size(0)} rows for a plan over {plan.n_src} source nodes")
        ctx.plan = plan
        out = torch.empty((plan.n, x.size(1)), dtype=torch.float32, device=x.device)
        if out.numel():
            with torch.cuda.device(x.device):
                _lib.check(_lib.load().hmp_segment_mean_fwd(x.data_ptr(), x.stride(0), x.size(1), plan.plan, out.data_ptr(),
                                                             out.stride(0), _lib.stream_ptr()))
        return out

    @staticmethod
    def backward(ctx, g):
        g = _rows(g)
        gx = torch.empty((ctx.plan.n_src, g.size(1)), dtype=torch.float32, device=g.device)
        if gx.numel() and ctx.plan.n == 0:
            gx.zero_()
        elif gx.numel():
            with torch.cuda.device(g.device):
                _lib.check(_lib.load().hmp_segment_mean_bwd(g.data_ptr(), g.stride(0), g.size(1), ctx.plan.plan, gx.data_ptr(),
                                                             gx.stride(0), _lib.stream_ptr()))
        return gx, None


def segment_mean(x: torch.Tensor, plan: GraphPlan) -> torch.Tensor:
    return _SegmentMean.apply(x, plan)


def project(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    return _Project.apply(x, weight)


def gcn_propagate(z: torch.Tensor, plan: GraphPlan) -> torch.Tensor:
    return _WSum.apply(z, plan, True, None)


def gin_propagate(z: torch.Tensor, plan: GraphPlan, eps: torch.Tensor) -> torch.Tensor:
    return _WSum.apply(z, plan, False, eps)


def bias_act_drop(x, bias=None, relu=False, p=0.0, seed=0, rng_step=0, rng_stream=0, elu=False) -> torch.Tensor:
    act = _lib.ACT_ELU if elu else (_lib.ACT_RELU if relu else _lib.ACT_NONE)
    return _BiasActDrop.apply(x, bias, act, p, seed, rng_step, rng_stream)


def batch_norm(x, gamma, beta, running_mean, running_var, momentum, eps, training) -> torch.Tensor:
    return _BatchNorm.apply(x, gamma, beta, running_mean, running_var, momentum, eps, training)


def argmax_rows(x: torch.Tensor) -> torch.Tensor:
    """``x.argmax(dim=1)`` (first maximum) as int64 on the device (``hmp_argmax_rows``)"""
    _dev(x, "x")
    x = _rows(x)
    out = torch.empty(x.size(0), dtype=torch.int64, device=x.device)
    if x.size(0):
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().hmp_argmax_rows(x.data_ptr(), x.stride(0), x.size(0), x.size(1), out.data_ptr(), _lib.stream_ptr()))
    return out


def predict_rows(logits: torch.Tensor, members: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``logits.argmax(dim=1)`` (first maximum) as int64 on the device, ``-1`` where the bool row filter ``members`` is False
    (``hmp_predict_rows``: the prediction :func:`count_correct_rows` compares).  ``out``: a contiguous int64 tensor of at least
    ``rows`` entries on the same device.  Nothing synchronises."""
    _dev(logits, "logits")
    logits = _rows(logits)
    if logits.dim() != 2 or logits.size(1) < 1:
        raise _lib.HydraMPError(f"logits must be [rows, classes >= 1], got {tuple(logits.shape)}")
    n = logits.size(0)
    members = row_members(members, n, logits.device)
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=logits.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.int64 or not out.is_contiguous() or out.device != logits.device
          or out.dim() != 1 or out.numel() < n):
        raise _lib.HydraMPError(f"out must be a contiguous 1-d int64 tensor on {logits.device} with at least {n} rows")
    if n:
        with torch.cuda.device(logits.device):
            _lib.check(_lib.load().hmp_predict_rows(logits.data_ptr(), logits.stride(0), n, logits.size(1),
                                                    members.data_ptr() if members is not None else None, out.data_ptr(),
                                                    _lib.stream_ptr()))
    return out[:n]


def topk_rows(logits: torch.Tensor, k: int, members: Optional[torch.Tensor] = None, out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(labels [rows, k] int64, probs [rows, k] float32)`` on the device (``hmp_topk_rows``): the k largest entries of every row
    -- descending, equal entries by ascending class, so column 0 is :func:`predict_rows`' label -- and their softmax probabilities.
    Columns past the class count, and rows where the bool filter ``members`` is False, hold ``-1`` / ``0``.  ``1 <= k <= 8``.
    ``out``: a ``(labels, probs)`` pair of contiguous tensors with k columns and at least ``rows`` rows on the same device.
    Nothing synchronises."""
    from .engine import _check_k, _topk_buffers

    k = _check_k(k)
    _dev(logits, "logits")
    logits = _rows(logits)
    if logits.dim() != 2 or logits.size(1) < 1:
        raise _lib.HydraMPError(f"logits must be [rows, classes >= 1], got {tuple(logits.shape)}")
    n = logits.size(0)
    members = row_members(members, n, logits.device)
    labels, probs = _topk_buffers(out, [n], k, False, logits.device)[0]
    if n:
        with torch.cuda.device(logits.device):
            _lib.check(_lib.load().hmp_topk_rows(logits.data_ptr(), logits.stride(0), n, logits.size(1),
                                                 members.data_ptr() if members is not None else None, k, labels.data_ptr(),
                                                 probs.data_ptr(), _lib.stream_ptr()))
    return labels[:n], probs[:n]


def mc_acc(rows: int, n_classes: int, device) -> torch.Tensor:
    """Monte-Carlo dropout accumulators of ``rows`` rows with ``n_classes`` classes: an uninitialised float32 ``[rows, ld]`` tensor on
    ``device`` with ``ld = hmp_mc_acc_ld(n_classes)`` (include/hydra_mp.h states the layout).  The first sample is stored
    (``first=True``), so nothing needs zeroing."""
    if isinstance(n_classes, bool) or not isinstance(n_classes, int) or n_classes < 1 or int(rows) < 0:
        raise _lib.HydraMPError(f"mc_acc: rows {rows!r} (>= 0), n_classes {n_classes!r} (>= 1)")
    return torch.empty((int(rows), int(_lib.load().hmp_mc_acc_ld(n_classes))), dtype=torch.float32, device=device)


def _check_mc_acc(acc, n_classes: int, device, who: str) -> None:
    if (not isinstance(acc, torch.Tensor) or acc.dtype != torch.float32 or acc.dim() != 2 or acc.device != device
            or (acc.size(0) > 1 and acc.stride(0) < acc.size(1)) or (acc.numel() and acc.stride(1) != 1)
            or acc.size(1) < int(_lib.load().hmp_mc_acc_ld(n_classes))):
        raise _lib.HydraMPError(f"{who}: acc must be a row-major float32 tensor [rows, >= hmp_mc_acc_ld({n_classes})] on {device} "
                                "(ops.mc_acc makes one)")


def _acc_ld(acc: torch.Tensor) -> int:
    return acc.stride(0) if acc.size(0) > 1 else acc.size(1)


def mc_accumulate_rows(logits: torch.Tensor, acc: torch.Tensor, first: bool, members: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One Monte-Carlo dropout sample (``hmp_mc_accumulate_rows``): the softmax of every row of ``logits`` -- bit-equal to
    :func:`topk_rows`' probabilities --, its squares and its entropy are ADDED to the row's accumulators in ``acc`` (from
    :func:`mc_acc`, one row per row of ``logits``), or STORED with ``first=True``.  Rows where the bool filter ``members`` is False
    are not touched.  Returns ``acc``; nothing synchronises."""
    _dev(logits, "logits")
    logits = _rows(logits)
    if logits.dim() != 2 or logits.size(1) < 1:
        raise _lib.HydraMPError(f"logits must be [rows, classes >= 1], got {tuple(logits.shape)}")
    n, n_classes = logits.size(0), logits.size(1)
    _check_mc_acc(acc, n_classes, logits.device, "mc_accumulate_rows")
    if acc.size(0) != n:
        raise _lib.HydraMPError(f"mc_accumulate_rows: acc has {acc.size(0)} rows, logits {n}")
    members = row_members(members, n, logits.device)
    if n:
        with torch.cuda.device(logits.device):
            _lib.check(_lib.load().hmp_mc_accumulate_rows(logits.data_ptr(), logits.stride(0) if n > 1 else n_classes, n, n_classes,
                                                          members.data_ptr() if members is not None else None, 1 if first else 0,
                                                          acc.data_ptr(), _acc_ld(acc), _lib.stream_ptr()))
    return acc


def mc_finish(acc: torch.Tensor, n_classes: int, samples: int, members: Optional[torch.Tensor] = None, out=None):
    """``(labels int64 [rows], mean_probs float32 [rows, n_classes], std, entropy, mutual_info float32 [rows])`` of ``samples``
    accumulated samples on the device (``hmp_mc_finish``): the mean predictive distribution, its first-maximum argmax, the standard
    deviation of the label's probability over the samples, the entropy of the mean and the mutual information between prediction
    and weights (entropy of the mean minus mean entropy, clamped at 0).  Rows where ``members`` is False hold ``-1`` / ``0``.
    ``out``: such a 5-tuple of contiguous tensors with at least ``rows`` rows on the same device.  Nothing synchronises."""
    from .engine import _check_samples, _mc_buffers

    samples = _check_samples(samples)
    if isinstance(n_classes, bool) or not isinstance(n_classes, int) or n_classes < 1:
        raise _lib.HydraMPError(f"mc_finish: n_classes {n_classes!r} (>= 1)")
    if not isinstance(acc, torch.Tensor) or not acc.is_cuda:
        raise _lib.HydraMPError("mc_finish: acc is not a device tensor; hydra_gnn_amd has no CPU fallback")
    _check_mc_acc(acc, n_classes, acc.device, "mc_finish")
    n = acc.size(0)
    members = row_members(members, n, acc.device)
    bufs = _mc_buffers(out, [n], [n_classes], False, acc.device)[0]
    if n:
        with torch.cuda.device(acc.device):
            _lib.check(_lib.load().hmp_mc_finish(acc.data_ptr(), _acc_ld(acc), n, n_classes, samples,
                                                 members.data_ptr() if members is not None else None, bufs[0].data_ptr(),
                                                 bufs[1].data_ptr(), n_classes, bufs[2].data_ptr(), bufs[3].data_ptr(),
                                                 bufs[4].data_ptr(), _lib.stream_ptr()))
    return tuple(b[:n] for b in bufs)


def check_count_buffers(counts: torch.Tensor, confusion: Optional[torch.Tensor], n_classes: int, device) -> None:
    """the accumulators of the room-task validation count: ``counts`` contiguous int64[>= 2], ``confusion`` (optional) contiguous
    int64 with ``n_classes ** 2`` elements, both on ``device``"""
    if (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int64 or counts.numel() < 2 or not counts.is_contiguous()
            or counts.device != device):
        raise _lib.HydraMPError(f"counts must be a contiguous int64[2] tensor on {device}")
    if confusion is not None and (confusion.dtype != torch.int64 or confusion.numel() != n_classes * n_classes
                                  or not confusion.is_contiguous() or confusion.device != device):
        raise _lib.HydraMPError(f"confusion must be a contiguous int64[{n_classes} * {n_classes}] tensor on {device}")


def row_members(members: Optional[torch.Tensor], n_rows: int, device) -> Optional[torch.Tensor]:
    """``members`` as the kernels read it: a contiguous bool tensor of ``n_rows`` entries on ``device`` (one byte per row)"""
    if members is None:
        return None
    if not isinstance(members, torch.Tensor) or members.dtype != torch.bool:
        raise _lib.HydraMPError("members must be a bool tensor (one entry per row)")
    if members.device != device:
        raise _lib.HydraMPError(f"members is on {members.device}, the rows are on {device}")
    if members.numel() != n_rows:
        raise _lib.HydraMPError(f"members: {members.numel()} entries for {n_rows} rows")
    return members.contiguous()


def count_correct_rows(logits: torch.Tensor, labels: torch.Tensor, counts: torch.Tensor, ignored_label: int = 25,
                       members: Optional[torch.Tensor] = None, confusion: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The per-batch arithmetic of ``BaseTrainingJob.test`` (``base_training_job.py:269-313``) on the device
    (``hmp_count_correct_rows``): ``pred = logits.argmax(dim=1)`` (first maximum); a row counts iff ``members[row]`` (all rows
    when None) and ``labels[row] != ignored_label``.  ADDS {correct, total} to ``counts`` (int64[2]) and, when given,
    ``confusion[label, pred] += 1`` to ``confusion`` (int64 [C, C] or [C * C]).  Returns ``counts``; nothing synchronises."""
    _dev(logits, "logits")
    logits = _rows(logits)
    if logits.dim() != 2 or logits.size(1) < 1:
        raise _lib.HydraMPError(f"logits must be [rows, classes >= 1], got {tuple(logits.shape)}")
    n, n_classes = logits.size(0), logits.size(1)
    dev = logits.device
    if not isinstance(labels, torch.Tensor) or labels.device != dev or labels.numel() != n:
        raise _lib.HydraMPError(f"labels must hold {n} entries on {dev}")
    labels = labels.to(torch.int64).contiguous()
    check_count_buffers(counts, confusion, n_classes, dev)
    members = row_members(members, n, dev)
    if n:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().hmp_count_correct_rows(
                logits.data_ptr(), logits.stride(0) if n > 1 else n_classes, n, n_classes, labels.data_ptr(),
                members.data_ptr() if members is not None else None, int(ignored_label), counts.data_ptr(),
                confusion.data_ptr() if confusion is not None else None, _lib.stream_ptr()))
    return counts


def check_graph_ptr(graph_ptr, n_rows: int, device) -> None:
    """the row offsets of a batch's graphs: a contiguous int64 ``[n_graphs + 1]`` tensor on ``device`` (``Batch.ptr``)"""
    if (not isinstance(graph_ptr, torch.Tensor) or graph_ptr.dtype != torch.int64 or graph_ptr.dim() != 1 or graph_ptr.numel() < 1
            or not graph_ptr.is_contiguous() or graph_ptr.device != device):
        raise _lib.HydraMPError(f"graph_ptr must be a contiguous int64 [n_graphs + 1] tensor on {device} (the row offsets of the "
                                "batch's graphs; a homogeneous Data batch carries none: pass graph_ptr=)")
    if graph_ptr.numel() < 2 and n_rows > 0:
        raise _lib.HydraMPError(f"graph_ptr describes no graph, the batch has {n_rows} rows")


def check_graph_counts(counts, n_graphs: int, device) -> None:
    if (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int64 or counts.numel() != 2 * n_graphs or not counts.is_contiguous()
            or counts.device != device):
        raise _lib.HydraMPError(f"counts must be a contiguous int64 [{n_graphs}, 2] tensor on {device} ({{correct, total}} per graph)")


def count_correct_rows_by_graph(logits: torch.Tensor, labels: torch.Tensor, counts: torch.Tensor, graph_ptr: torch.Tensor,
                                ignored_label: int = 25, members: Optional[torch.Tensor] = None) -> torch.Tensor:
    """:func:`count_correct_rows` per graph (``hmp_count_correct_rows_by_graph``): the rows of graph ``g`` are
    ``[graph_ptr[g], graph_ptr[g + 1])`` (device int64 ``[n_graphs + 1]``, ``graph_ptr[-1] == rows``); ADDS {correct, total} of
    graph ``g`` to ``counts[g]`` (int64 ``[n_graphs, 2]``).  Returns ``counts``; nothing synchronises."""
    _dev(logits, "logits")
    logits = _rows(logits)
    if logits.dim() != 2 or logits.size(1) < 1:
        raise _lib.HydraMPError(f"logits must be [rows, classes >= 1], got {tuple(logits.shape)}")
    n, n_classes = logits.size(0), logits.size(1)
    dev = logits.device
    if not isinstance(labels, torch.Tensor) or labels.device != dev or labels.numel() != n:
        raise _lib.HydraMPError(f"labels must hold {n} entries on {dev}")
    labels = labels.to(torch.int64).contiguous()
    check_graph_ptr(graph_ptr, n, dev)
    n_graphs = graph_ptr.numel() - 1
    check_graph_counts(counts, n_graphs, dev)
    members = row_members(members, n, dev)
    if n:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().hmp_count_correct_rows_by_graph(
                logits.data_ptr(), logits.stride(0) if n > 1 else n_classes, n, n_classes, labels.data_ptr(),
                members.data_ptr() if members is not None else None, int(ignored_label), graph_ptr.data_ptr(), n_graphs,
                counts.data_ptr(), _lib.stream_ptr()))
    return counts
