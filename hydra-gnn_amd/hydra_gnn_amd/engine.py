"""Host side of the native network executor (``hmp_net_*`` in ``include/hydra_mp.h``).

:class:`NativeNet` turns a model description (node/edge types, per-layer convs with their
``nn.Parameter`` objects) into an ``hmp_net_spec``, keeps all parameters in ONE flat fp32 buffer
(the named parameters are views into it, so ``state_dict()`` keeps the reference's PyG keys while
the optimiser / all-reduce see one contiguous tensor), owns the device workspace and exposes

* ``forward(data)`` -- autograd-compatible (one ``torch.autograd.Function`` around
  ``hmp_net_forward`` / ``hmp_net_backward``), so the reference's training loop
  (``loss.backward(); opt.step()``, ``src/hydra_gnn/base_training_job.py:202-216``) works unchanged;
* :class:`TrainStep` -- the same loop body as two native phases (fwd+loss+bwd, Adam) captured in
  hipGraphs, with one flat gradient all-reduce between them for data parallelism.

torch is used for device memory, streams and ``torch.distributed`` only.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib
from ._lib import ACT_ELU, ACT_NONE, ACT_RELU, CONV_GAT, CONV_SAGE

EdgeType = Tuple[str, str, str]


class ConvDesc:
    """One conv of one layer: kind, edge type and its parameters (by role)."""

    def __init__(self, kind: int, edge_type: EdgeType, f_out: int, params: Dict[str, Optional[nn.Parameter]], **gat):
        self.kind, self.edge_type, self.f_out, self.params = kind, tuple(edge_type), f_out, params
        self.gat = gat  # heads, concat, self_loops, edge_dim, fill_mean, shared_lin
        self.active = True


class LayerDesc:
    def __init__(self, convs: List[ConvDesc], out_dims: Dict[str, int], act: int, dropout: float, group_mean: bool = False,
                 passthrough: Sequence[str] = ()):
        self.convs, self.out_dims, self.act, self.dropout, self.group_mean = convs, out_dims, act, dropout, group_mean
        # first layer only: node types whose input features stay visible to the next layer (`x_dict.update(pre_mp(..))`)
        self.passthrough = list(passthrough)


def _require_cuda(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise _lib.HydraMPError(
            f"{what} is on {t.device}: hydra_gnn_amd runs on MI355X (cuda/HIP device) only and has no CPU fallback"
        )


SEL_ALL, SEL_MASK, SEL_ORDINAL = 0, 1, 2  # include/hydra_mp.h: HMP_SEL_*
WRT_CODES = {"logit": 0, "logprob": 1}  # HMP_WRT_*
SAL_MAX_GROUPS = 4  # csrc/kernels.h
DEFAULT_GROUPS = ((0, 3), (3, 6), (6, None))  # position, box size, word2vec block of the 306-d object features


class _PtrView:
    """an int64 vector that lives inside a buffer someone else keeps alive (a stream's collated ``ptr``), known by address"""

    def __init__(self, addr: int):
        self.addr = addr

    def data_ptr(self) -> int:
        return self.addr


class _HostMirror:
    """A device byte buffer, its pinned host twin and one event: a call's results land in ``dev``, cross in ONE device-to-host copy
    and are read through views of ``host``, which stay valid until the next call that uses the mirror."""

    def __init__(self):
        self.dev = self.host = self.done = None

    def reserve(self, nbytes: int, device) -> bool:
        """at least ``nbytes`` on ``device`` (a grown buffer takes twice the need, 4096 at the least); True: the buffers are new"""
        if self.dev is not None and self.dev.numel() >= nbytes and self.dev.device == device:
            return False
        cap = max(4096, 2 * nbytes)
        self.dev = torch.empty(cap, dtype=torch.uint8, device=device)
        self.host = torch.empty(cap, dtype=torch.uint8).pin_memory()
        self.done = torch.cuda.Event()
        return True

    def fetch(self, nbytes: int) -> torch.Tensor:
        """the first ``nbytes`` bytes down in one copy, one event recorded and waited for; returns them (a view of ``host``)"""
        host = self.host[:nbytes]
        if nbytes > 0:
            host.copy_(self.dev[:nbytes], non_blocking=True)
        self.done.record()
        self.done.synchronize()
        return host


def _pairs(buf: torch.Tensor, n: int):
    """the int64 and float32 halves of a mirror buffer that holds ``n`` 8-byte entries, then ``n`` 4-byte ones"""
    return buf[:8 * n].view(torch.int64), buf[8 * n:12 * n].view(torch.float32)


class _BatchHolder:
    """ctypes batch descriptor + the tensors it points at (kept alive while kernels run)."""

    def __init__(self):
        self.c = _lib.Batch()
        self.keep: List[torch.Tensor] = []
        self.n_nodes: List[int] = []
        self.n_edges: List[int] = []
        self.edge_tensors: List[torch.Tensor] = []
        # an input had to be copied (dtype / layout conversion): the descriptor points at a private copy, so it must not be
        # reused for a later step (in-place edits of the caller's tensor would be missed)
        self.converted = False
        # store.BatchStream that owns the descriptor (device-collated batches): it holds the targets of a two-headed stream
        self.stream = None
        # node type index -> largest row count of one graph of the batch, where the collation knows it on the host
        self.max_rows: Dict[int, int] = {}


_NO_CLASS_W = ()  # the unweighted step's (empty) class-weight tuple: compared by identity


class NativeNet:
    _class_w = _NO_CLASS_W  # set_class_weights: the vectors the library currently borrows (one per head)

    def __init__(self, node_types: Sequence[str], in_dims: Dict[str, int], edge_types: Sequence[EdgeType],
                 layers: List[LayerDesc], readout: str, pool_edge_type: Optional[EdgeType] = None,
                 count_types: Sequence[str] = (), aux_readout: Optional[str] = None, tail: Optional[Tuple[int, float]] = None,
                 heads: Optional[Sequence[nn.Linear]] = None, head_pools: Optional[Sequence[Optional[EdgeType]]] = None):
        self.node_types = list(node_types)
        self.edge_types = [tuple(e) for e in edge_types]
        self.in_dims = dict(in_dims)
        self.layers = layers
        self.readout = readout
        # second output node type of the two-headed task (heterogeneous_network.py:123-135): forward returns (readout, aux)
        self.aux_readout = aux_readout
        assert aux_readout is None or (aux_readout != readout and pool_edge_type is None)
        # (activation, dropout) the two-headed model applies to both final states after the program (heterogeneous_network.py:
        # 124-134); only the fused two-head step (TwoHeadTrainStep) and count_correct run it natively
        self.tail = (int(tail[0]), float(tail[1])) if tail is not None else (ACT_NONE, 0.0)
        # two LEARNED linear heads (room, object) over the readout's final state (homogeneous_network.py:138-147): their
        # parameters live in the flat buffer inside [0, n_active) so one all-reduce and Adam cover them, but they are not part of
        # `params` (the autograd path of forward() computes the heads in torch and never returns their gradients)
        self.heads = list(heads) if heads is not None else None
        assert self.heads is None or (len(self.heads) == 2 and aux_readout is None)
        self.head_params: List[nn.Parameter] = []
        self.pool_edge_type = tuple(pool_edge_type) if pool_edge_type is not None else None
        # two-headed nets whose heads read a LeafPool of their final state (heterogeneous_neural_tree_network.py:186-205): the pool
        # edge type of (readout, aux), None = unpooled; labels and masks then have one row per node of the edge type's destination
        self.head_pools = None
        if head_pools is not None:
            assert aux_readout is not None and len(head_pools) == 2
            self.head_pools = tuple(tuple(e) if e is not None else None for e in head_pools)
            for e, t in zip(self.head_pools, (readout, aux_readout)):
                assert e is None or (e in [tuple(x) for x in edge_types] and e[0] == t)
        # node types without features whose node COUNT matters (virtual pool targets)
        self.count_types = list(count_types)
        assert len(self.node_types) <= _lib.MAX_NODE_TYPES and len(self.edge_types) <= _lib.MAX_EDGE_TYPES
        # edge types whose convs read edge attributes (GAT_edge) -> attribute width
        self.edge_dims: Dict[EdgeType, int] = {}
        for layer in layers:
            for conv in layer.convs:
                d = int(conv.gat.get("edge_dim", 0) or 0)
                if d:
                    self.edge_dims[conv.edge_type] = d
        self._mark_liveness()
        self._layout_params()
        self._handle = None
        self._ws = None
        self._caps = None
        self._flat: Optional[torch.Tensor] = None
        self._lib = None
        self._fwd_token = 0
        self._compute_bf16 = False
        self._plan_key = None  # versions of the edge lists whose plan the workspace holds (predict() reuses it across frames)
        self._plan_tensors = None  # ... and the edge tensors themselves (identity is the test; holding them pins their addresses)
        self._agg_first: Dict[Tuple[int, int], bool] = {}  # (layer, conv) -> evaluated aggregate-first (decided with the first batch)
        # the host results of predict / predict_pair, of predict_confidence, and of explain / explain_salient
        self._pred, self._conf, self._att = _HostMirror(), _HostMirror(), _HostMirror()
        self._conf_views = None  # predict_confidence: (rows per head, device views, host views) of the last call
        # predict_mc: the accumulators of each head (regrown on demand); predict_uncertainty: its host results
        self._mc_cache: List[Optional[torch.Tensor]] = [None, None]
        self._unc = _HostMirror()

    def set_compute(self, precision: str) -> None:
        """'fp32' (default): every projection on the exact fp32 MFMA path.  'bf16': GEMM calls in the throughput-bound regime
        (>= 1024 64x64 output tiles, i.e. BASELINE config 5) round their operands to bf16 and accumulate in fp32; storage stays
        fp32.  An explicit precision choice: outside the 1e-5 parity bar of the fp32 path."""
        if precision not in ("fp32", "bf16"):
            raise ValueError("precision must be 'fp32' or 'bf16'")
        self._compute_bf16 = precision == "bf16"
        if self._handle is not None:
            _lib.check(self._lib.hmp_net_set_compute(self._handle, int(self._compute_bf16)))

    # ---- static analysis ---------------------------------------------------------------------
    def _mark_liveness(self) -> None:
        """A conv is live iff its output can reach the readout (reference computes the others and
        throws them away: heterogeneous_network.py:121-122).  Dead convs keep their parameters
        (state_dict compatible) but receive no gradient, exactly like ``grad is None`` in torch."""
        needed = {self.readout} | ({self.aux_readout} if self.aux_readout is not None else set())
        for layer in reversed(self.layers):
            nxt = set()
            for conv in layer.convs:
                s, _, t = conv.edge_type
                conv.active = t in needed
                if conv.active:
                    nxt.update((s, t))
            nxt.update(t for t in layer.passthrough if t in needed)
            needed = nxt

    def _layout_params(self) -> None:
        roles = ("w0", "w1", "w2", "a0", "a1", "a2", "b0")
        seen: Dict[int, int] = {}
        order: List[Tuple[nn.Parameter, bool]] = []
        for active_pass in (True, False):
            for layer in self.layers:
                for conv in layer.convs:
                    for r in roles:
                        p = conv.params.get(r)
                        if p is None or id(p) in seen:
                            continue
                        live = conv.active and self._role_used(conv, r)
                        if live != active_pass:
                            continue
                        seen[id(p)] = len(order)
                        order.append((p, live))
            if active_pass and self.heads is not None:  # after the live conv parameters, in front of the dead ones
                for lin in self.heads:
                    for p in (lin.weight, lin.bias):
                        seen[id(p)] = len(order)
                        order.append((p, None))
        # a parameter shared by several convs (GAT lin_src == lin_dst) is active if any user is
        off = 0
        self.param_offsets: Dict[int, int] = {}
        self.params: List[nn.Parameter] = []
        self.param_active: List[bool] = []
        for p, live in order:
            self.param_offsets[id(p)] = off
            if live is None:
                self.head_params.append(p)
                live = True
            else:
                self.params.append(p)
                self.param_active.append(live)
            off += ((p.numel() + 3) // 4) * 4  # keep every tensor 16-byte aligned in the flat buffer
            if live:
                self.n_active = off
        if not any(self.param_active):
            self.n_active = 0
        self.n_params = off

    @staticmethod
    def _role_used(conv: ConvDesc, role: str) -> bool:
        if conv.kind == CONV_SAGE:
            return role in ("w0", "b0", "w1")
        # GAT: lin_dst of a same-type conv built from a tuple is never used
        s, _, t = conv.edge_type
        if role == "w1" and s == t and not conv.gat.get("shared_lin", False):
            return False
        return True

    # ---- native objects ------------------------------------------------------------------------
    def _spec(self) -> _lib.NetSpec:
        sp = _lib.NetSpec()
        nt = {t: i for i, t in enumerate(self.node_types)}
        et = {e: i for i, e in enumerate(self.edge_types)}
        sp.n_node_types, sp.n_edge_types, sp.n_layers = len(self.node_types), len(self.edge_types), len(self.layers)
        for t, i in nt.items():
            sp.in_dim[i] = int(self.in_dims.get(t, 0))
        for e, i in et.items():
            sp.edge_src[i], sp.edge_dst[i] = nt[e[0]], nt[e[2]]
        sp.readout_type = nt[self.readout]
        sp.pool_edge_type = et[self.pool_edge_type] if self.pool_edge_type is not None else -1
        sp.aux_readout_type = nt[self.aux_readout] if self.aux_readout is not None else -1
        sp.n_params, sp.n_active_params = self.n_params, self.n_active
        sp.tail_act, sp.tail_dropout = self.tail
        for l, layer in enumerate(self.layers):
            ls = sp.layers[l]
            ls.n_convs, ls.act, ls.dropout, ls.group_mean = len(layer.convs), layer.act, float(layer.dropout), int(layer.group_mean)
            for t, i in nt.items():
                ls.out_dim[i] = int(layer.out_dims.get(t, 0))
                ls.passthrough[i] = int(t in layer.passthrough)
            for c, conv in enumerate(layer.convs):
                cs = ls.convs[c]
                cs.kind, cs.edge_type = conv.kind, et[conv.edge_type]
                cs.src, cs.dst, cs.f_out = nt[conv.edge_type[0]], nt[conv.edge_type[2]], conv.f_out
                cs.heads = int(conv.gat.get("heads", 1))
                cs.concat = int(conv.gat.get("concat", 0))
                cs.self_loops = int(conv.gat.get("self_loops", 0))
                cs.edge_dim = int(conv.gat.get("edge_dim", 0) or 0)
                cs.fill_mean = int(conv.gat.get("fill_mean", 0))
                cs.shared_lin = int(conv.gat.get("shared_lin", 0))
                cs.active = int(conv.active)
                cs.agg_first = int(self._agg_first.get((l, c), False))
                cs.att_dropout = float(conv.gat.get("dropout", 0.0) or 0.0)
                for r in ("w0", "w1", "w2", "a0", "a1", "a2", "b0"):
                    p = conv.params.get(r)
                    setattr(cs, r, self.param_offsets[id(p)] if p is not None else -1)
        return sp

    def _decide_agg_first(self, h: Optional["_BatchHolder"]) -> None:
        """Which SAGE convs are evaluated in the reference's own order -- mean of the source rows, then ``lin_l`` on the (few)
        destination rows ([PyG] SAGEConv) -- instead of projecting every source row first (both are exact).
        Decided ONCE, from the sizes of the first batch the handle is built for (the choice is part of the executor's static
        layout): a conv between two node types whose source type is large (>= 32 768 rows) and at least 16x the destination type,
        with at most two edges per source row -- objects -> rooms at 10^6 objects; at most one per source type and layer.
        ``HMP_AGG_FIRST=0`` never, ``=1`` every eligible conv whatever the sizes (tests)."""
        self._agg_first = {}
        mode = os.environ.get("HMP_AGG_FIRST")
        if mode == "0" or (h is None and mode != "1"):
            return
        nt = {t: i for i, t in enumerate(self.node_types)}
        et = {e: i for i, e in enumerate(self.edge_types)}
        for l, layer in enumerate(self.layers):
            taken = set()
            for c, conv in enumerate(layer.convs):
                s, _, t = conv.edge_type
                if conv.kind != CONV_SAGE or not conv.active or s == t or s in taken:
                    continue
                if mode != "1":
                    ns, nd, ne = h.n_nodes[nt[s]], h.n_nodes[nt[t]], h.n_edges[et[conv.edge_type]]
                    if not (ns >= 32768 and ns >= 16 * max(nd, 1) and 0 < ne <= 2 * ns):
                        continue
                self._agg_first[(l, c)] = True
                taken.add(s)

    def _ensure_handle(self, h: Optional["_BatchHolder"] = None):
        if self._handle is None:
            self._lib = _lib.require_device()
            self._decide_agg_first(h)
            h = C.c_void_p()
            sp = self._spec()
            _lib.check(self._lib.hmp_net_create(C.byref(sp), C.byref(h)))
            self._handle = h
            if self._compute_bf16:
                _lib.check(self._lib.hmp_net_set_compute(h, 1))
            if self.heads is not None:
                _lib.check(self._lib.hmp_net_set_linear_heads(h, C.byref(self._linear_heads())))
            if self.head_pools is not None:
                ets = [self.edge_types.index(e) if e is not None else -1 for e in self.head_pools]
                _lib.check(self._lib.hmp_net_set_head_pools(h, *ets))
            self._push_class_weights()
        return self._handle

    # ---- class weights of the cross entropy ----------------------------------------------------------
    def head_classes(self) -> Tuple[int, ...]:
        """class count of every head: (readout,) or (readout / rooms, aux / objects)"""
        if self.heads is not None:
            return tuple(int(lin.out_features) for lin in self.heads)
        out = self.layers[-1].out_dims
        if self.aux_readout is not None:
            return int(out[self.readout]), int(out[self.aux_readout])
        return (int(out[self.readout]),)

    def set_class_weights(self, weights) -> None:
        """``weights``: one float32 device vector (or None) per head -- the class weights of every later training step of this
        net (``hmp_net_set_class_weights``; the library borrows the pointers, this object keeps the tensors alive)."""
        self._class_w = weights
        if self._handle is not None:
            self._push_class_weights()

    def _push_class_weights(self) -> None:
        ws = tuple(self._class_w)
        for head in range(2):  # a head without an entry is cleared
            w = ws[head] if head < len(ws) else None
            _lib.check(self._lib.hmp_net_set_class_weights(self._handle, head, w.data_ptr() if w is not None else None,
                                                           w.numel() if w is not None else 0))

    def head_label_types(self) -> Tuple[str, str]:
        """node types whose rows carry the labels of the (readout, aux) heads: the pool destination of a pooled head"""
        pools = self.head_pools or (None, None)
        return tuple(e[2] if e is not None else t for e, t in zip(pools, (self.readout, self.aux_readout)))

    def _linear_heads(self) -> _lib.LinearHeads:
        hd = _lib.LinearHeads()
        hd.F = int(self.heads[0].in_features)
        for k, lin in enumerate(self.heads):
            hd.classes[k] = int(lin.out_features)
            hd.w_off[k] = self.param_offsets[id(lin.weight)]
            hd.b_off[k] = self.param_offsets[id(lin.bias)]
        return hd

    def __del__(self):
        try:
            if self._handle is not None and self._lib is not None:
                self._lib.hmp_net_destroy(self._handle)
        except Exception:
            pass

    # ---- flat parameters -------------------------------------------------------------------------
    def flat_params(self, full_check: bool = True) -> torch.Tensor:
        """The flat fp32 buffer the named parameters are views of (re-created after ``.to()``)."""
        p0 = self.params[0]
        _require_cuda(p0.data, "model parameters")
        ok = self._flat is not None and self._flat.device == p0.device
        if ok:
            base = self._flat.data_ptr()
            # `.to()` / `.float()` re-home every parameter; the first and the last one are checked on the hot path (one call
            # per step), all of them when the check is forced
            probe = self.params + self.head_params if full_check else (self.params[0], self.params[-1])
            for p in probe:
                if p.data.data_ptr() != base + 4 * self.param_offsets[id(p)] or p.dtype != torch.float32:
                    ok = False
                    break
        if not ok:
            flat = torch.zeros(self.n_params + 4, dtype=torch.float32, device=p0.device)
            for p in self.params + self.head_params:
                if p.dtype != torch.float32:
                    raise _lib.HydraMPError("hydra_gnn_amd computes in fp32: parameter dtype must be float32")
                off = self.param_offsets[id(p)]
                view = flat[off:off + p.numel()].view(p.shape)
                view.copy_(p.data)
                p.data = view
            self._flat = flat
        return self._flat

    # ---- batch + workspace -------------------------------------------------------------------------
    def make_batch(self, data, labels: Optional[torch.Tensor] = None) -> _BatchHolder:
        h = _BatchHolder()
        x_dict = data.x_dict
        ei_dict = data.edge_index_dict
        for i, t in enumerate(self.node_types):
            if t in x_dict and self.in_dims.get(t, 0) > 0:
                x = x_dict[t]
                _require_cuda(x, f"x_dict['{t}']")
                if x.dtype != torch.float32 or x.stride(-1) != 1 or (x.dim() == 2 and x.size(0) > 1 and x.stride(0) < x.size(1)):
                    x = x.to(torch.float32).contiguous()
                    h.converted = True
                if x.size(1) != self.in_dims[t]:
                    raise _lib.HydraMPError(f"x_dict['{t}'] has {x.size(1)} features, model expects {self.in_dims[t]}")
                h.keep.append(x)
                h.c.n_nodes[i] = x.size(0)
                h.c.d_x[i] = x.data_ptr()
                h.c.ldx[i] = x.stride(0) if x.size(0) > 1 else x.size(1)
            else:
                h.c.n_nodes[i] = int(data[t].num_nodes) if t in self.count_types or t in x_dict else 0
            h.n_nodes.append(int(h.c.n_nodes[i]))
        for i, e in enumerate(self.edge_types):
            if e in ei_dict:
                ei = ei_dict[e]
                _require_cuda(ei, f"edge_index_dict[{e}]")
                if ei.dtype != torch.int64 or not ei.is_contiguous():
                    ei = ei.to(torch.int64).contiguous()
                    h.converted = True
                h.keep.append(ei)
                h.edge_tensors.append(ei)
                h.c.n_edges[i] = ei.size(1)
                h.c.d_edge_index[i] = ei.data_ptr() if ei.size(1) > 0 else None
            else:
                # PyG's HeteroConv SKIPS a conv whose edge type is absent from the dict (no root / bias term, smaller group-mean
                # divisor), which differs from a present-but-empty `[2, 0]` edge_index.  The reference's loaders always
                # materialise every type (`fill_missing_edge_index`, mp3d_dataset.py:220-255); the executor's stacked operands
                # are built for the full conv set, so an absent key is refused instead of silently computing something else.
                raise _lib.HydraMPError(
                    f"edge_index_dict has no entry for {e}: pass an empty [2, 0] int64 edge_index for edge types without "
                    "edges (the reference does: fill_missing_edge_index, mp3d_dataset.py:220-255)")
            h.n_edges.append(int(h.c.n_edges[i]))
        if self.edge_dims:
            ea_dict = data.edge_attr_dict
            for i, e in enumerate(self.edge_types):
                d = self.edge_dims.get(e, 0)
                if d == 0 or h.n_edges[i] == 0:
                    continue
                if e not in ea_dict:
                    raise _lib.HydraMPError(f"edge_attr_dict[{e}] is required by the GAT_edge convs")
                ea = ea_dict[e]
                _require_cuda(ea, f"edge_attr_dict[{e}]")
                if ea.dtype != torch.float32 or not ea.is_contiguous():
                    ea = ea.to(torch.float32).contiguous()
                    h.converted = True
                if ea.dim() != 2 or ea.size(0) != h.n_edges[i] or ea.size(1) != d:
                    raise _lib.HydraMPError(f"edge_attr_dict[{e}] must be [{h.n_edges[i]}, {d}], got {tuple(ea.shape)}")
                h.keep.append(ea)
                h.c.d_edge_attr[i] = ea.data_ptr()
        nt = {t: i for i, t in enumerate(self.node_types)}
        out_type = self.pool_edge_type[2] if self.pool_edge_type is not None else self.readout
        h.c.n_out = h.n_nodes[nt[out_type]]
        # the batch as a union of graphs ([PyG] Batch.ptr per node store + the collation's host-side maximum): optional
        mg = int(getattr(data, "max_graph_nodes", 0) or 0)
        ng = 0
        if mg > 0:
            for i, t in enumerate(self.node_types):
                st_ = data[t] if t in x_dict else None
                p = getattr(st_, "ptr", None) if st_ is not None else None
                if p is None or not p.is_cuda or p.dtype != torch.int64 or not p.is_contiguous() or int(p[-1:].numel()) == 0:
                    if h.n_nodes[i] > 0:
                        ng = 0
                        break
                    continue
                if ng and p.numel() - 1 != ng:
                    ng = 0
                    break
                ng = p.numel() - 1
                h.keep.append(p)
                h.c.d_node_ptr[i] = p.data_ptr()
        h.c.n_graphs = ng
        h.c.max_graph_nodes = mg if ng else 0
        if ng:
            rows = getattr(data, "max_graph_rows", None) or {}
            h.max_rows = {i: int(rows[t]) for i, t in enumerate(self.node_types) if t in rows}
        if ng:  # graph-sorted edge lists (collate's per-edge-type ptr)
            for i, e in enumerate(self.edge_types):
                st_ = data[e] if e in data.edge_types else None
                p = getattr(st_, "ptr", None) if st_ is not None else None
                # `ptr` vouches for ONE edge_index (data.collate stamps its version): an edge list edited in place since then is
                # described without it (any edge order accepted; a replaced edge_index dropped `ptr` already)
                pv = getattr(st_, "ptr_version", None) if st_ is not None else None
                if pv is not None and int(h.edge_tensors[i]._version) != int(pv):
                    p = None
                if p is not None and p.is_cuda and p.dtype == torch.int64 and p.is_contiguous() and p.numel() == ng + 1:
                    h.keep.append(p)
                    h.c.d_edge_ptr[i] = p.data_ptr()
        if labels is not None:
            _require_cuda(labels, "labels")
            lab = labels.to(torch.int64).contiguous()
            if lab is not labels:
                h.converted = True
            if lab.numel() != h.c.n_out:
                raise _lib.HydraMPError(f"{lab.numel()} labels for {h.c.n_out} output rows")
            h.keep.append(lab)
            h.c.d_labels = lab.data_ptr()
        return h

    def _ensure_workspace(self, h: _BatchHolder, device) -> None:
        handle = self._ensure_handle(h)
        need_n, need_e = h.n_nodes, h.n_edges
        if self._caps is not None and self._ws is not None and self._ws.device == device:
            cn, ce = self._caps
            if all(a <= b for a, b in zip(need_n, cn)) and all(a <= b for a, b in zip(need_e, ce)):
                return
            need_n = [max(a, b) for a, b in zip(need_n, cn)]
            need_e = [max(a, b) for a, b in zip(need_e, ce)]
        cn = [max(1, int(v)) for v in need_n]
        ce = [max(1, int(v)) for v in need_e]
        cn_c = (C.c_int32 * len(cn))(*cn)
        ce_c = (C.c_int64 * len(ce))(*ce)
        nbytes = int(self._lib.hmp_net_workspace_bytes(handle, cn_c, ce_c))
        torch.cuda.synchronize(device)
        self._ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _lib.check(self._lib.hmp_net_bind_workspace(handle, self._ws.data_ptr(), nbytes, cn_c, ce_c))
        self._caps = (cn, ce)
        self._fwd_token += 1  # activations of an earlier forward are gone: its backward must fail loudly

    def _ws_view(self, ptr: int, rows: int, ld: int) -> torch.Tensor:
        off = ptr - self._ws.data_ptr()
        assert 0 <= off and off + rows * ld * 4 <= self._ws.numel() and off % 4 == 0
        return self._ws[off:off + rows * ld * 4].view(torch.float32).view(rows, ld)

    # ---- autograd-compatible forward -------------------------------------------------------------
    def forward(self, data, training: bool, seed: int = 0, rng_step: int = 0) -> torch.Tensor:
        flat = self.flat_params()
        h = self.make_batch(data)
        # inputs that ask for a gradient ([PyG] idiom: x.requires_grad_(); model(data)[i, c].backward(); x.grad) become inputs of
        # the autograd node, behind the parameters; without one the call is what it always was
        h.grad_inputs = []
        xs = []
        if torch.is_grad_enabled():
            x_dict = data.x_dict
            for i, t in enumerate(self.node_types):
                x = x_dict.get(t) if self.in_dims.get(t, 0) > 0 else None
                if x is not None and x.requires_grad:
                    if x.dtype != torch.float32:
                        raise _lib.HydraMPError(f"x_dict['{t}'] requires a gradient: it must be float32 (hydra_gnn_amd computes in fp32)")
                    h.grad_inputs.append(i)
                    xs.append(x)
        with torch.cuda.device(flat.device):
            self._ensure_workspace(h, flat.device)
            return _NetFunction.apply(self, h, bool(training), int(seed), int(rng_step), *self.params, *xs)

    # ---- inference hot loop (bin/room_classification_server:273-299) -------------------------------------------------
    def predict(self, data, n_classes: int) -> torch.Tensor:
        """``forward(data).argmax(dim=1).cpu()`` of the reference's ``GnnModel.infer`` without autograd, without copying the
        logits and with ONE small D2H: eval-mode native forward, ``hmp_argmax_rows`` on the executor's output, labels into a
        pinned host buffer.  Returns a host int64 tensor (a view of that buffer: valid until the next call)."""
        flat = self.flat_params(full_check=False)
        h = self.make_batch(data)
        dev = flat.device
        n = int(h.c.n_out)
        with torch.cuda.device(dev):
            self._ensure_workspace(h, dev)
            self._pred.reserve(8 * n, dev)
            out_p, ld = C.c_void_p(), C.c_int32()
            st = _lib.stream_ptr()
            # consecutive frames with the SAME edge tensors (unchanged in place): the plan of the previous call is reused
            # (bin/room_classification_server:273-299 re-infers on a graph whose topology did not change)
            # "same" = the very same tensor OBJECTS as the previous call (kept alive in `_plan_tensors`, so the allocator cannot
            # hand their addresses to a new frame's edge lists) at the same `_version`: a fresh tensor that merely lands on a
            # recycled address rebuilds the plan
            key = None if h.converted else (id(self._ws), tuple(h.n_nodes), tuple(t._version for t in h.edge_tensors))
            prev = self._plan_tensors
            same = (key is not None and key == self._plan_key and prev is not None and len(prev) == len(h.edge_tensors)
                    and all(a is b for a, b in zip(prev, h.edge_tensors)))
            h.c.plan_valid = 1 if same else 0
            _lib.check(self._lib.hmp_net_forward(self._handle, C.byref(h.c), flat.data_ptr(), 0, 0, 0, C.byref(out_p), C.byref(ld), st))
            self._fwd_token += 1
            self._plan_key = key
            self._plan_tensors = list(h.edge_tensors) if key is not None else None
            if n > 0:
                _lib.check(self._lib.hmp_argmax_rows(out_p.value, ld.value, n, int(n_classes), self._pred.dev.data_ptr(), st))
            return self._pred.fetch(8 * n).view(torch.int64)

    def count_correct(self, data, labels, masks, counts: torch.Tensor) -> torch.Tensor:
        """Two-headed nets: ADD this batch's {correct, total} of both heads to the device int64[4] ``counts`` (``hmp_net_count_correct2``:
        eval-mode forward, argmax of act(final state), comparison under the masks).  Nothing synchronises."""
        flat = self.flat_params(full_check=False)
        h = self.make_batch(data)
        _check_counts4(counts, flat.device)
        tg = _head_targets(self, h, labels, masks)
        self._count("hmp_net_count_correct2", h, flat.device, C.byref(tg), flat.data_ptr(), counts.data_ptr())
        return counts

    def count_correct_stream(self, holder: "_BatchHolder", mask: Optional[str], counts: torch.Tensor) -> torch.Tensor:
        """:meth:`count_correct` / :meth:`count_correct_heads` on a device-collated batch of a two-headed stream
        (``store.BatchStream.next``): labels, head rows and the mask called ``mask`` are the stream's own.  Nothing synchronises."""
        stream = getattr(holder, "stream", None)
        if stream is None or stream.nat is not self:
            raise _lib.HydraMPError("count_correct: the batch descriptor does not come from a stream created for this model")
        flat = self.flat_params(full_check=False)
        _check_counts4(counts, flat.device)
        entry = "hmp_net_count_correct_heads" if self.heads is not None else "hmp_net_count_correct2"
        self._count(entry, holder, flat.device, stream.targets(mask), flat.data_ptr(), counts.data_ptr())
        return counts

    def count_correct_heads(self, data, labels, mask, members, counts: torch.Tensor) -> torch.Tensor:
        """Nets with linear heads: ADD this batch's {correct, total} of both heads to the device int64[4] ``counts``
        (``hmp_net_count_correct_heads``: eval-mode forward, argmax of both heads on act(final state), comparison under ``mask``
        on the member rows).  Nothing synchronises."""
        flat = self.flat_params(full_check=False)
        h = self.make_batch(data)
        _check_counts4(counts, flat.device)
        tg = _linear_head_targets(self, h, labels, mask, members)
        self._count("hmp_net_count_correct_heads", h, flat.device, C.byref(tg), flat.data_ptr(), counts.data_ptr())
        return counts

    def count_correct_rooms(self, batch, labels, counts: torch.Tensor, ignored_label: int = 25,
                            members: Optional[torch.Tensor] = None, confusion: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Room task: ADD this batch's {correct, total} to the device int64[2] ``counts`` and, when given, its confusion matrix to
        the device int64[C * C] ``confusion`` (``hmp_net_count_correct_rooms``: eval-mode forward, first-maximum argmax of the
        output, comparison with ``labels`` on the rows of ``members`` whose label is not ``ignored_label``).  ``batch`` is a data
        object or a descriptor from ``store.BatchStream.next``, which brings its own labels (pass ``labels=None``).  Nothing
        synchronises."""
        h, members_ptr, flat = self._room_batch("count_correct_rooms", batch, labels, members, ignored_label)
        dev = flat.device
        from .ops import check_count_buffers

        check_count_buffers(counts, confusion, self.n_classes, dev)
        self._count("hmp_net_count_correct_rooms", h, dev, flat.data_ptr(), members_ptr, int(ignored_label), counts.data_ptr(),
                    confusion.data_ptr() if confusion is not None else None)
        return counts

    def _room_batch(self, what: str, batch, labels, members, ignored_label: int):
        """(descriptor, address of the row filter or None, flat parameters) of a room-task count on a data object with ``labels``
        or on a stream descriptor, which brings its labels and -- a stream of homogeneous graphs -- its ``room_mask`` rows and
        ignored label"""
        if self.aux_readout is not None or self.heads is not None:
            raise _lib.HydraMPError(f"{what}: a two-headed net counts with count_correct / count_correct_heads")
        flat = self.flat_params(full_check=False)
        if isinstance(batch, _BatchHolder):
            if labels is not None:
                raise _lib.HydraMPError(f"{what}: a stream batch brings its own labels (pass labels=None)")
            h = batch
            stream = h.stream
            if stream is not None and getattr(stream, "homog_room", False):
                if stream.nat is not self:
                    raise _lib.HydraMPError(f"{what}: the batch comes from a stream created for another model")
                if int(ignored_label) != stream.ignored_label:
                    raise _lib.HydraMPError(f"{what}: ignored_label {ignored_label}, but the stream wrote its labels with ignored_label "
                                            f"{stream.ignored_label} outside room_mask")
                if members is None:
                    return h, stream.members.data_ptr(), flat
        else:
            if labels is None:
                raise _lib.HydraMPError(f"{what}: labels are required for a data batch")
            h = self.make_batch(batch, labels)
        if not h.c.d_labels and int(h.c.n_out) > 0:
            raise _lib.HydraMPError(f"{what}: the batch has no labels")
        from .ops import row_members

        members = row_members(members, int(h.c.n_out), flat.device)
        return h, (members.data_ptr() if members is not None else None), flat

    def count_correct_rooms_by_graph(self, batch, labels, counts: torch.Tensor, ignored_label: int = 25,
                                     members: Optional[torch.Tensor] = None, graph_ptr: Optional[torch.Tensor] = None) -> torch.Tensor:
        """:meth:`count_correct_rooms` per graph (``hmp_net_count_correct_rooms_by_graph``: one eval-mode forward, one count
        launch): ADD {correct, total} of graph ``g`` of the batch to ``counts[g]`` (device int64 ``[n_graphs, 2]``).  A stream
        descriptor brings the graphs' row offsets; a data batch needs ``graph_ptr``, the device int64 ``[n_graphs + 1]`` offsets of
        the output rows (``Batch.ptr`` of their node type).  Nothing synchronises."""
        h, members_ptr, flat = self._room_batch("count_correct_rooms_by_graph", batch, labels, members, ignored_label)
        dev = flat.device
        if not isinstance(batch, _BatchHolder):
            from .ops import check_graph_ptr

            check_graph_ptr(graph_ptr, int(h.c.n_out), dev)
            ng = graph_ptr.numel() - 1
            out_type = self.pool_edge_type[2] if self.pool_edge_type is not None else self.readout
            if int(h.c.n_graphs) not in (0, ng):
                raise _lib.HydraMPError(f"count_correct_rooms_by_graph: graph_ptr describes {ng} graphs, the batch {int(h.c.n_graphs)}")
            # the offsets of the output rows alone: without edge offsets the plan build reads the batch as before
            h.keep.append(graph_ptr)
            h.c.d_node_ptr[self.node_types.index(out_type)] = graph_ptr.data_ptr()
            h.c.n_graphs = ng
        from .ops import check_graph_counts

        check_graph_counts(counts, int(h.c.n_graphs), dev)
        self._count("hmp_net_count_correct_rooms_by_graph", h, dev, flat.data_ptr(), members_ptr, int(ignored_label),
                    counts.data_ptr())
        return counts

    def predict_labels(self, batch, out=None, members=None):
        """The labels the count entries compare, on the device: eval-mode native forward plus ONE launch (``hmp_net_predict_rooms``
        / ``hmp_net_predict2`` / ``hmp_net_predict_heads``, picked by the net's kind).  ``batch`` is a data object or a descriptor
        from ``store.BatchStream.next``; no labels are needed.

        * room task: an int64 tensor with a label per output row, ``-1`` where ``members`` (a bool row filter; a stream of
          homogeneous graphs brings its ``room_mask`` rows) is False;
        * two-headed net with an aux readout: a pair, one label per row of ``head_label_types()`` (pooled heads: per pooled row);
        * linear heads: a pair of per-row vectors, ``-1`` outside each head's rows.  ``members = (room rows, object rows | None)``
          for a data batch (None = the complement of the room rows); a two-headed stream brings its own.

        ``out`` takes caller-owned contiguous device int64 buffers (one, or a pair) of at least the needed rows; the result is a
        view of their leading rows.  Nothing synchronises."""
        h, stream, flat, rows = self._label_rows(batch, "predict_labels")
        dev = flat.device
        two = len(rows) == 2
        outs = _label_buffers(out, rows, two, dev)
        mem, _alive = self._label_members(h, stream, members, rows, dev, "predict_labels")
        self._label_entry("predict", h, flat, mem, (), [outs])
        views = tuple(o[:n] for o, n in zip(outs, rows))
        return views if two else views[0]

    def _label_entry(self, what: str, h, flat, mem, extra: tuple, outputs) -> None:
        """``hmp_net_<what>_rooms`` / ``2`` / ``_heads`` by the net's kind: the parameters, the members (an aux-readout net has
        none), ``extra``, then every output's address -- of a two-headed net, the pair of its heads' addresses"""
        kind = "_heads" if self.heads is not None else "2" if self.aux_readout is not None else "_rooms"
        outs = [ts[0].data_ptr() if kind == "_rooms" else (C.c_void_p * 2)(*[t.data_ptr() for t in ts]) for ts in outputs]
        self._count(f"hmp_net_{what}{kind}", h, flat.device, flat.data_ptr(), *(() if kind == "2" else (mem,)), *extra, *outs)

    def _label_rows(self, batch, who: str):
        """(holder, its stream or None, flat parameters, rows per head) of a label call: one entry for the room task, two for a
        two-headed net"""
        h, flat = self._readout_batch(batch, who)
        stream = h.stream  # None for a data batch
        if self.heads is not None:
            rows = [int(h.c.n_out)] * 2
        elif self.aux_readout is not None:
            rows = [h.n_nodes[self.node_types.index(t)] for t in self.head_label_types()]
        else:
            rows = [int(h.c.n_out)]
        return h, stream, flat, rows

    def _label_members(self, h, stream, members, rows, dev, who: str):
        """the member argument of the net kind's label entry (a pair of row addresses for linear heads, one address or None for the
        room task, None for an aux-readout net) and the tensors that must outlive the call"""
        from .ops import row_members

        if self.heads is not None:
            keep = None
            if stream is not None and members is None:
                m0, m1 = stream.member_rows()
            else:
                if members is None or len(members) != 2 or members[0] is None:
                    raise _lib.HydraMPError(f"{who}: a net with linear heads needs members=(room rows, object rows | None)")
                keep = [row_members(m, rows[0], dev) if m is not None else None for m in members]
                m0, m1 = (k.data_ptr() if k is not None and rows[0] > 0 else None for k in keep)
            return (C.c_void_p * 2)(m0, m1), keep
        if self.aux_readout is not None:
            if members is not None:
                raise _lib.HydraMPError(f"{who}: the heads of an aux-readout net are whole node types (no members)")
            return None, None
        if members is None and stream is not None and getattr(stream, "homog_room", False):
            return stream.members.data_ptr(), None
        members = row_members(members, rows[0], dev)
        return (members.data_ptr() if members is not None else None), members

    def predict_topk(self, batch, k: int, out=None, members=None):
        """Top-k labels with their softmax probabilities, on the device: eval-mode native forward plus ONE launch
        (``hmp_net_topk_rooms`` / ``hmp_net_topk2`` / ``hmp_net_topk_heads``, picked by the net's kind as :meth:`predict_labels`
        picks, with its ``batch`` and ``members``).  ``1 <= k <= 8``.

        Per head ``(labels [rows, k] int64, probs [rows, k] float32)``: ``labels[r, j]`` is the class with the j-th largest score
        of what ``forward()`` returns for the row in eval mode (equal scores: the smaller class), ``probs[r, j]`` its softmax
        probability; column 0 is :meth:`predict_labels`' label.  Columns past the class count, and every column of a row outside
        the head's rows, hold ``-1`` / ``0``.  The room task returns one such pair, a two-headed net a pair of them.

        ``out`` takes caller-owned buffers of that shape (``(labels, probs)``, or a pair of those): contiguous, on the model's
        device, k columns, at least the needed rows; the result is a view of their leading rows.  Nothing synchronises."""
        k = _check_k(k)
        h, stream, flat, rows = self._label_rows(batch, "predict_topk")
        dev = flat.device
        two = len(rows) == 2
        outs = _topk_buffers(out, rows, k, two, dev)
        mem, _alive = self._label_members(h, stream, members, rows, dev, "predict_topk")
        self._label_entry("topk", h, flat, mem, (k,), [[o[0] for o in outs], [o[1] for o in outs]])
        views = tuple((lb[:n], pb[:n]) for (lb, pb), n in zip(outs, rows))
        return views if two else views[0]

    def predict_confidence(self, batch, members=None):
        """:meth:`predict_topk` with ``k = 1`` on the host: the labels and their probabilities of every head land in ONE device
        buffer (8 bytes per label, then 4 per probability) and cross in one D2H through one pinned buffer and one event, as
        :meth:`predict_pair` moves its labels.  Returns host ``(labels int64 [rows], confidence float32 [rows])`` per head -- one
        pair for the room task, a pair of pairs for a two-headed net -- as views of that buffer (valid until the next call)."""
        h, _, flat, rows = self._label_rows(batch, "predict_confidence")
        dev = flat.device
        n = sum(rows)
        with torch.cuda.device(dev):
            fresh = self._conf.reserve(12 * n, dev)
            if fresh or self._conf_views is None or self._conf_views[0] != rows:  # consecutive frames of one size reuse the views

                def split(buf):
                    lab, prb = _pairs(buf, n)
                    return [(lab[o:o + r], prb[o:o + r]) for o, r in zip((0, rows[0]), rows)]

                outs = [(lb.view(lb.numel(), 1), pb.view(pb.numel(), 1)) for lb, pb in split(self._conf.dev)]
                host = split(self._conf.host)
                self._conf_views = (list(rows), tuple(outs) if len(rows) == 2 else outs[0], tuple(host) if len(rows) == 2 else host[0])
            _, outs, host = self._conf_views
            self.predict_topk(h, 1, out=outs, members=members)
            self._conf.fetch(12 * n)
        return host

    # ---- Monte-Carlo dropout uncertainty ---------------------------------------------------------------------------------
    def _mc_accs(self, rows: Sequence[int], classes: Sequence[int], dev) -> List[torch.Tensor]:
        """the cached accumulators of :meth:`predict_mc`, one ``[rows, hmp_mc_acc_ld(C)]`` view per head; a buffer is regrown when a
        batch needs more floats than it holds"""
        cache = self._mc_cache
        views = []
        for i, (n, c) in enumerate(zip(rows, classes)):
            ld = int(self._lib.hmp_mc_acc_ld(c))
            buf = cache[i]
            if buf is None or buf.numel() < n * ld or buf.device != dev:
                buf = cache[i] = torch.empty(max(2 * n * ld, 1024), dtype=torch.float32, device=dev)
            views.append(buf[:n * ld].view(n, ld))
        return views

    def _mc_finish_members(self, h, stream, mem, keep, rows):
        """the member address of every head's finishing launch (None: every row) and what must outlive it: the room task's row
        filter, nothing for the whole node types of an aux-readout net, the member rows of linear heads -- the object head's being
        the complement of the room rows where the net has no object rows of its own"""
        if self.heads is None:
            return ([mem] if self.aux_readout is None else [None, None]), None
        m0, m1 = mem[0], mem[1]
        alive = None
        if m1 is None and rows[0] > 0:
            room = stream.room_rows()[:rows[0]] if keep is None else keep[0]
            alive = ~room
            m1 = alive.data_ptr()
        return [m0, m1], alive

    def predict_mc(self, batch, samples: int, seed: int, first_step: int = 1, members=None, out=None):
        """Monte-Carlo dropout on the device: ``samples`` = T stochastic passes, sample ``t`` being the training-mode forward at the
        dropout site ``(seed, first_step + t)`` -- feature, attention and tail dropout all draw -- plus ONE launch that adds the
        softmax of the sample's scores to per-row accumulators (``hmp_net_mc_rooms`` / ``hmp_net_mc2`` / ``hmp_net_mc_heads``, picked
        by the net's kind as :meth:`predict_labels` picks, with its ``batch`` and ``members``), then one finishing launch per head
        (``hmp_mc_finish``).  ``1 <= samples <= 4096``, ``0 <= first_step``, ``first_step + samples <= 2**32``.

        Per head ``(labels int64 [rows], mean_probs float32 [rows, C], std, entropy, mutual_info float32 [rows])``: the mean
        predictive distribution over the samples, its first-maximum argmax, the standard deviation of that label's probability, the
        entropy of the mean and the mutual information between prediction and weights (entropy of the mean minus the mean entropy).
        Rows outside the head's rows hold ``-1`` / ``0``.  The room task returns one such tuple, a two-headed net a pair of them.

        ``out`` takes caller-owned buffers of that structure (contiguous, on the model's device, at least the needed rows); the result
        is a view of their leading rows.  The accumulators are cached on the net.  Nothing synchronises; the parameters are read,
        never written."""
        samples = _check_samples(samples)
        first_step = _check_first_step(first_step, samples)
        seed = _check_seed(seed)
        h, stream, flat, rows = self._label_rows(batch, "predict_mc")
        dev = flat.device
        two = len(rows) == 2
        classes = self.head_classes()
        outs = _mc_buffers(out, rows, classes, two, dev)
        mem, keep = self._label_members(h, stream, members, rows, dev, "predict_mc")
        self._ensure_handle(h)
        with torch.cuda.device(dev):
            accs = self._mc_accs(rows, classes, dev)
            fin, _alive = self._mc_finish_members(h, stream, mem, keep, rows)
        kind = "_heads" if self.heads is not None else "2" if self.aux_readout is not None else "_rooms"
        if kind == "_rooms":
            acc_args = (accs[0].data_ptr(), accs[0].size(1))
        else:
            acc_args = ((C.c_void_p * 2)(*[a.data_ptr() if a.numel() else None for a in accs]), (C.c_int32 * 2)(*[a.size(1) for a in accs]))
        for t in range(samples):
            self._count(f"hmp_net_mc{kind}", h, dev, flat.data_ptr(), *(() if kind == "2" else (mem,)), seed, first_step + t,
                        1 if t == 0 else 0, *acc_args)
        with torch.cuda.device(dev):
            for a, c, n, m, o in zip(accs, classes, rows, fin, outs):
                if n:
                    _lib.check(self._lib.hmp_mc_finish(a.data_ptr(), a.size(1), n, c, samples, m, o[0].data_ptr(), o[1].data_ptr(), c,
                                                       o[2].data_ptr(), o[3].data_ptr(), o[4].data_ptr(), _lib.stream_ptr()))
        views = tuple(tuple(t[:n] for t in o) for o, n in zip(outs, rows))
        return views if two else views[0]

    def predict_uncertainty(self, batch, samples: int, seed: int, first_step: int = 1, members=None):
        """:meth:`predict_mc` on the host: every output of every head lands in ONE device buffer (8 bytes per label, then the
        floats) and crosses in one D2H through one pinned buffer and one event, as :meth:`predict_confidence` moves its pairs.
        Returns host ``(labels int64 [rows], mean_probs float32 [rows, C], std, entropy, mutual_info float32 [rows])`` per head --
        one tuple for the room task, a pair for a two-headed net -- as views of that buffer (valid until the next call)."""
        h, _, flat, rows = self._label_rows(batch, "predict_uncertainty")
        dev = flat.device
        classes = self.head_classes()
        n_lab = sum(rows)
        nbytes = 8 * n_lab + 4 * sum(n * (c + 3) for n, c in zip(rows, classes))
        mirror = self._unc

        def split(buf):
            heads, lo, fo = [], 0, 8 * n_lab
            for n, c in zip(rows, classes):
                lab = buf[lo:lo + 8 * n].view(torch.int64)
                lo += 8 * n
                fl = buf[fo:fo + 4 * n * (c + 3)].view(torch.float32)
                fo += 4 * n * (c + 3)
                heads.append((lab, fl[:n * c].view(n, c), fl[n * c:n * c + n], fl[n * c + n:n * c + 2 * n], fl[n * c + 2 * n:]))
            return tuple(heads) if len(rows) == 2 else heads[0]

        with torch.cuda.device(dev):
            mirror.reserve(nbytes, dev)
            self.predict_mc(h, samples, seed, first_step, members=members, out=split(mirror.dev))
            mirror.fetch(nbytes)
        return split(mirror.host)

    def predict_pair(self, batch, members=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """:meth:`predict_labels` of a two-headed net on the host: both label vectors land in ONE device buffer and cross in one
        D2H through one pinned buffer and one event, as :meth:`predict` does for the room task.  Returns host int64 views of that
        buffer (valid until the next call)."""
        if self.aux_readout is None and self.heads is None:
            raise _lib.HydraMPError("predict_pair: the net has one output; use predict()")
        h, _, flat, rows = self._label_rows(batch, "predict_pair")
        dev = flat.device
        n = rows[0] + rows[1]
        with torch.cuda.device(dev):
            self._pred.reserve(8 * n, dev)
            pred = self._pred.dev[:8 * n].view(torch.int64)
            self.predict_labels(h, out=(pred[:rows[0]], pred[rows[0]:]), members=members)
            host = self._pred.fetch(8 * n).view(torch.int64)
        return host[:rows[0]], host[rows[0]:]

    # ---- attention export ([PyG] GATConv.forward(return_attention_weights=True)) -------------------------------------
    def _gat_layer(self, layer: int, who: str) -> List[ConvDesc]:
        """the convs of program layer ``layer`` after the checks that it exists and is a GAT layer"""
        if isinstance(layer, bool) or not isinstance(layer, int) or not 0 <= layer < len(self.layers):
            raise _lib.HydraMPError(f"{who}: layer {layer!r} out of range (the program has {len(self.layers)} layers)")
        convs = self.layers[layer].convs
        if not convs or convs[0].kind != CONV_GAT:
            raise _lib.HydraMPError(f"{who}: no attention coefficients: layer {layer} is not a GAT layer")
        return convs

    def _gat_conv(self, layer: int, edge_type, who: str) -> ConvDesc:
        """the live GAT conv of program layer ``layer`` on ``edge_type``, or the refusal that names what is wrong"""
        for conv in self._gat_layer(layer, who):
            if conv.edge_type == tuple(edge_type):
                if not conv.active:
                    raise _lib.HydraMPError(f"{who}: the conv on edge type {conv.edge_type} of layer {layer} is inactive: its output "
                                            "never reaches the readout, so nothing is computed for it")
                return conv
        raise _lib.HydraMPError(f"{who}: layer {layer} has no conv on edge type {tuple(edge_type)!r}")

    def attention_edge_types(self, layer: int) -> List[EdgeType]:
        """edge types of the live GAT convs of program layer ``layer`` (what :meth:`attention` exports by default)"""
        return [c.edge_type for c in self._gat_layer(layer, "attention") if c.active]

    def _readout_batch(self, batch, who: str):
        """(descriptor, flat parameters) of a label, attention or saliency call on a data object or on a stream descriptor"""
        flat = self.flat_params(full_check=False)
        if isinstance(batch, _BatchHolder):
            h = batch
            if h.stream is not None and h.stream.nat is not self:
                raise _lib.HydraMPError(f"{who}: the batch comes from a stream created for another model")
        else:
            h = self.make_batch(batch)
        return h, flat

    def attention_rows(self, h: _BatchHolder, conv: ConvDesc) -> Tuple[int, int, int]:
        """(E, n_loop, n_dst) of ``conv`` on the batch ``h``: alpha has ``E + n_loop`` rows, the top-k outputs ``n_dst``"""
        ns, nd = (h.n_nodes[self.node_types.index(t)] for t in (conv.edge_type[0], conv.edge_type[2]))
        n_loop = min(ns, nd) if conv.gat.get("self_loops", 0) else 0
        return h.n_edges[self.edge_types.index(conv.edge_type)], n_loop, nd

    def attention(self, batch, layer: int, edge_types=None, out=None) -> Dict[EdgeType, torch.Tensor]:
        """Attention coefficients of program layer ``layer``, on the device: eval-mode native forward plus ONE launch
        (``hmp_net_attention``).  ``batch`` is a data object or a descriptor from ``store.BatchStream.next``.

        Returns ``{edge_type: alpha}`` for ``edge_types`` (default: every live conv of the layer), ``alpha`` float32
        ``[E + n_loop, heads]``: row ``e < E`` belongs to column ``e`` of the batch's ``edge_index``, row ``E + i`` to the self loop
        ``i -> i`` the conv appends (``n_loop = min(n_src, n_dst)`` for a conv with self loops, else 0); an input edge ``i -> i``
        such a conv removes, and an edge dropped for an out-of-range endpoint, hold 0.  The values are the pre-dropout softmax
        weights the backward differentiates.

        ``out`` takes caller-owned buffers ``{edge_type: tensor}``: contiguous float32 on the model's device, ``heads`` columns,
        at least the needed rows; the result is a view of their leading rows.  Nothing synchronises."""
        ets = [tuple(e) for e in edge_types] if edge_types is not None else self.attention_edge_types(layer)
        convs = [self._gat_conv(layer, e, "attention") for e in ets]
        h, flat = self._readout_batch(batch, "attention")
        dev = flat.device
        slots = (C.c_void_p * _lib.MAX_EDGE_TYPES)()
        res = {}
        for conv in convs:
            E, n_loop, _ = self.attention_rows(h, conv)
            H = int(conv.gat.get("heads", 1))
            buf = _attention_buffer(out.get(conv.edge_type) if out is not None else None, E + n_loop, H, torch.float32, dev,
                                    f"out[{conv.edge_type}]")
            slots[self.edge_types.index(conv.edge_type)] = buf.data_ptr()
            res[conv.edge_type] = buf[:E + n_loop]
        self._count("hmp_net_attention", h, dev, flat.data_ptr(), int(layer), slots, 1, None, None)
        return res

    def top_attended(self, batch, layer: int, edge_type, k: int, out=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The ``k`` most attended sources of every destination row of the conv on ``edge_type`` in program layer ``layer``, on the
        device: eval-mode native forward plus ONE launch (``hmp_net_attention``).  ``1 <= k <= 8``.

        Returns ``(src int64 [n_dst, k], weight float32 [n_dst, k])``: the entries with the largest head-mean coefficient (heads
        added in ascending order in float32, divided by the head count), descending; equal means by ascending original edge id,
        the appended self loop last.  ``src`` is the source node index (the row itself for the loop).  Removed and dropped edges
        are no candidates; columns past a row's live entries hold ``-1`` / ``0``.

        ``out`` takes caller-owned ``(src, weight)`` buffers: contiguous, on the model's device, ``k`` columns, at least ``n_dst``
        rows; the result is a view of their leading rows.  Nothing synchronises.

        ``edge_type`` may also be a LIST of edge types: the same single launch serves them all and the result is
        ``{edge_type: (src, weight)}`` (``out`` then a dict of pairs)."""
        k = _check_k(k)
        many = isinstance(edge_type, list)
        convs = [self._gat_conv(layer, e, "top_attended") for e in (edge_type if many else [edge_type])]
        h, flat = self._readout_batch(batch, "top_attended")
        dev = flat.device
        s_slots, w_slots = (C.c_void_p * _lib.MAX_EDGE_TYPES)(), (C.c_void_p * _lib.MAX_EDGE_TYPES)()
        res = {}
        for conv in convs:
            o = (out.get(conv.edge_type) if out is not None else None) if many else out
            if o is not None and (not isinstance(o, (tuple, list)) or len(o) != 2):
                raise _lib.HydraMPError("top_attended: out must be a (src, weight) pair of tensors")
            nd = self.attention_rows(h, conv)[2]
            src = _attention_buffer(o[0] if o is not None else None, nd, k, torch.int64, dev, "out[0]")
            wgt = _attention_buffer(o[1] if o is not None else None, nd, k, torch.float32, dev, "out[1]")
            i = self.edge_types.index(conv.edge_type)
            s_slots[i], w_slots[i] = src.data_ptr(), wgt.data_ptr()
            res[conv.edge_type] = (src[:nd], wgt[:nd])
        self._count("hmp_net_attention", h, dev, flat.data_ptr(), int(layer), None, k, s_slots, w_slots)
        return res if many else res[convs[0].edge_type]

    def explain(self, batch, layer: int, edge_type, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """:meth:`top_attended` on the host: sources and weights land in ONE device buffer (8 bytes per source, then 4 per weight)
        and cross in one D2H through one pinned buffer and one event, as :meth:`predict_confidence` moves its labels.  Returns host
        ``(src int64 [n_dst, k], weight float32 [n_dst, k])`` as views of that buffer (valid until the next call)."""
        k = _check_k(k)
        conv = self._gat_conv(layer, edge_type, "explain")
        h, flat = self._readout_batch(batch, "explain")
        dev = flat.device
        nd = self.attention_rows(h, conv)[2]
        n = nd * k
        with torch.cuda.device(dev):
            self._att.reserve(12 * n, dev)
            split = lambda buf: tuple(v.view(nd, k) for v in _pairs(buf, n))  # noqa: E731
            self.top_attended(h, layer, conv.edge_type, k, out=split(self._att.dev) if n > 0 else None)
            return split(self._att.fetch(12 * n))

    # ---- gradient saliency ([PyG] idiom: x.requires_grad_(); model(data)[i, c].backward(); x.grad) --------------------
    def _saliency_checks(self, who: str, wrt, head, rows, ordinal) -> Tuple[int, int]:
        """the argument checks of the saliency calls that need no device: (wrt code, head)"""
        if self.heads is not None:
            raise _lib.HydraMPError(f"{who}: nets with learned linear heads are not supported: their outputs are computed behind the "
                                    "native program (the homogeneous two-headed task)")
        if self._compute_bf16:
            raise _lib.HydraMPError(f"{who}: bf16 compute mode is not supported: input gradients are computed in fp32 "
                                    "(set_compute('fp32'))")
        if wrt not in WRT_CODES:
            raise _lib.HydraMPError(f"{who}: wrt must be 'logit' or 'logprob', got {wrt!r}")
        if isinstance(head, bool) or head not in (0, 1) or (head == 1 and self.aux_readout is None):
            raise _lib.HydraMPError(f"{who}: head {head!r}: " + ("0 (the readout) or 1 (the second output)" if self.aux_readout is not None
                                                                  else "the net has one output (head 0)"))
        if self.head_pools is not None:
            raise _lib.HydraMPError(f"{who}: two-headed nets with pooled heads are not supported")
        if rows is not None and ordinal is not None:
            raise _lib.HydraMPError(f"{who}: rows and ordinal overlap: pass one row selection")
        if ordinal is not None:
            p = ordinal[0] if isinstance(ordinal, (tuple, list)) and len(ordinal) == 2 else ordinal
            if isinstance(p, bool) or not isinstance(p, int) or p < 0:
                raise _lib.HydraMPError(f"{who}: ordinal must be an int >= 0 or (int >= 0, graph ptr), got {ordinal!r}")
        return WRT_CODES[wrt], int(head)

    def head_type(self, head: int = 0) -> str:
        """node type whose rows are the output rows of ``head``"""
        if head == 1:
            return self.aux_readout
        return self.pool_edge_type[2] if self.pool_edge_type is not None else self.readout

    def _head_rows(self, h: _BatchHolder, head: int) -> int:
        return int(h.c.n_out) if head == 0 else h.n_nodes[self.node_types.index(self.aux_readout)]

    def graph_ptr(self, h: _BatchHolder, node_type: str, dev) -> Tuple[torch.Tensor, int]:
        """(int64 ``ptr`` [G + 1] on the device, G) of ``node_type`` in the batch ``h``: the collation's, else one graph"""
        i = self.node_types.index(node_type)
        ng = int(h.c.n_graphs)
        if ng > 0 and h.c.d_node_ptr[i]:
            return _PtrView(int(h.c.d_node_ptr[i])), ng
        n = h.n_nodes[i]
        one = torch.arange(0, n + 1, n, dtype=torch.int64, device=dev) if n > 0 else torch.zeros(2, dtype=torch.int64, device=dev)
        return one, 1

    def _selection(self, h: _BatchHolder, head: int, rows, ordinal, dev, who: str):
        """(mode, mask address, ordinal, ptr address, graphs, tensors to keep alive) of a row selection over the rows of ``head``"""
        from .ops import row_members

        n = self._head_rows(h, head)
        if rows is not None:
            m = row_members(rows, n, dev)
            return SEL_MASK, (m.data_ptr() if n > 0 else None), 0, None, 0, m
        if ordinal is not None:
            if isinstance(ordinal, (tuple, list)):
                p, ptr = ordinal
                if (not isinstance(ptr, torch.Tensor) or ptr.dtype != torch.int64 or ptr.device != dev or ptr.dim() != 1 or ptr.numel() < 2
                        or not ptr.is_contiguous()):
                    raise _lib.HydraMPError(f"{who}: the graph ptr of ordinal must be a contiguous int64 vector [graphs + 1] on {dev}")
                ng = ptr.numel() - 1
            else:
                p = ordinal
                ptr, ng = self.graph_ptr(h, self.head_type(head), dev)
            return SEL_ORDINAL, None, int(p), ptr.data_ptr(), ng, ptr
        return SEL_ALL, None, 0, None, 0, None

    def _gx_buffers(self, h: _BatchHolder, out, dev, who: str):
        """per node type with input features: (index, gx storage [n, ldx], view [n, F]); ``out``: the caller's ``{type: tensor}``"""
        res = []
        for i, t in enumerate(self.node_types):
            F = self.in_dims.get(t, 0)
            if F <= 0 or not h.c.d_x[i]:
                continue
            n, ld = h.n_nodes[i], int(h.c.ldx[i])
            o = out.get(t) if out is not None else None
            if o is None:
                buf = torch.zeros((max(n, 1), ld), dtype=torch.float32, device=dev)  # types the program never reads keep 0
            else:
                if (not isinstance(o, torch.Tensor) or o.dtype != torch.float32 or o.device != dev or o.dim() != 2 or o.size(0) < n
                        or o.size(1) < F or o.stride(1) != 1 or (o.size(0) > 1 and o.stride(0) != ld)):
                    got = f"{tuple(o.shape)} {o.dtype} on {o.device}" if isinstance(o, torch.Tensor) else repr(type(o))
                    raise _lib.HydraMPError(f"{who}: out['{t}'] must be a float32 tensor [rows >= {n}, >= {F}] on {dev} with the row "
                                            f"pitch of x ({ld}), got {got}")
                buf = o
            res.append((i, t, buf, buf[:n, :F]))
        return res

    def input_gradients(self, batch, target=None, rows=None, ordinal=None, wrt: str = "logit", head: int = 0,
                        out=None) -> Dict[str, torch.Tensor]:
        """``{node_type: d s / d x[node_type]}`` on the device, float32 ``[n_t, F_t]``, where ``s`` is the sum over the selected
        output rows of ``head`` of the chosen class's logit (``wrt="logit"``) or log-probability (``"logprob"``): eval-mode native
        forward, one seed launch and the backward chain without the weight gradients (``hmp_net_input_gradient``).  Nothing
        synchronises; the activations of any earlier ``forward()`` are overwritten.

        ``target``: int64 class per output row on the device (a value outside ``[0, classes)`` falls back to the prediction);
        None: every row's own prediction (:meth:`predict_labels`).  Row selection: ``rows`` (a bool tensor over the output rows)
        or ``ordinal`` (``p``: the ``p``-th output row of every graph of the batch, by the collation's ``ptr``; ``(p, ptr)`` with
        an explicit int64 ``[G + 1]``); neither: all rows.  ``batch`` is a data object or a ``store.BatchStream`` descriptor.
        ``out``: caller-owned ``{node_type: tensor}`` with the row pitch of that type's ``x``, zeroed once by the caller (a node
        type the program never reads is not written)."""
        who = "input_gradients"
        w, head = self._saliency_checks(who, wrt, head, rows, ordinal)
        h, flat = self._readout_batch(batch, who)
        dev = flat.device
        n_out = self._head_rows(h, head)
        tgt = None
        if target is not None:
            _require_cuda(target, "target")
            if target.dtype != torch.int64 or target.numel() != n_out or target.device != dev:
                raise _lib.HydraMPError(f"{who}: target must be an int64 tensor with {n_out} entries on {dev}")
            tgt = target.contiguous()
        mode, mptr, p, pptr, ng, keep = self._selection(h, head, rows, ordinal, dev, who)
        bufs = self._gx_buffers(h, out, dev, who)
        slots = (C.c_void_p * _lib.MAX_NODE_TYPES)()
        for i, _, buf, _ in bufs:
            slots[i] = buf.data_ptr()
        self._count("hmp_net_input_gradient", h, dev, flat.data_ptr(), head, tgt.data_ptr() if tgt is not None and n_out > 0 else None,
                    mode, mptr, p, pptr, ng, w, slots)
        del keep
        return {t: view for _, t, _, view in bufs}

    def _score_ranges(self, groups, F: int, who: str):
        groups = tuple(groups) if groups is not None else ()
        if len(groups) > SAL_MAX_GROUPS:
            raise _lib.HydraMPError(f"{who}: {len(groups)} column groups (at most {SAL_MAX_GROUPS})")
        lo, hi = [], []
        for g in groups:
            if not isinstance(g, (tuple, list)) or len(g) != 2:
                raise _lib.HydraMPError(f"{who}: a column group is (lo, hi) with hi None = the last column, got {g!r}")
            lo.append(max(0, int(g[0])))
            hi.append(F if g[1] is None else min(F, int(g[1])))
        return lo, hi

    def saliency_scores(self, gx: torch.Tensor, x_ptr: int, ldx: int, n: int, F: int, groups, dev, who: str = "saliency"):
        """``(gxi [n], gnorm [n], groups [n, n_groups])`` of one node type: ``hmp_saliency_scores`` on a gradient view ``gx``
        (``[n, F]``, any pitch) against the input rows at ``x_ptr`` / ``ldx``"""
        lo, hi = self._score_ranges(groups, F, who)
        ng = len(lo)
        rows = max(n, 1)
        buf = torch.empty(rows * (2 + ng), dtype=torch.float32, device=dev)  # one allocation: gxi, gnorm, then the groups
        gxi, gnorm, grp = buf[:rows], buf[rows:2 * rows], buf[2 * rows:].view(rows, ng)
        lo_c, hi_c = (C.c_int32 * max(ng, 1))(*lo), (C.c_int32 * max(ng, 1))(*hi)
        with torch.cuda.device(dev):
            _lib.check(self._lib.hmp_saliency_scores(gx.data_ptr(), gx.stride(0) if gx.size(0) > 1 else max(gx.size(1), F), x_ptr, ldx, n, F, ng,
                                                     lo_c, hi_c, gxi.data_ptr(), gnorm.data_ptr(), grp.data_ptr() if ng else None,
                                                     _lib.stream_ptr()))
        return gxi[:n], gnorm[:n], grp[:n]

    def saliency(self, batch, groups=DEFAULT_GROUPS, **kw) -> Dict[str, Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]:
        """``{node_type: (gxi [n], gnorm [n], groups [n, n_groups])}`` on the device: :meth:`input_gradients` (``**kw``) reduced
        against the input per node row (``hmp_saliency_scores``, one launch per node type): ``gxi = sum_f g * x`` (signed gradient
        x input), ``gnorm = sqrt(sum_f g^2)``, ``groups[:, i]`` = gradient x input over the columns ``[lo, hi)`` of
        ``groups[i]`` (at most 4; ``hi`` None = the last column; clipped to the type's width).  The default groups are the blocks
        of the 306-d object features: position, box size, word2vec.  Nothing synchronises."""
        self._score_ranges(groups, 1, "saliency")
        self._saliency_checks("saliency", kw.get("wrt", "logit"), kw.get("head", 0), kw.get("rows"), kw.get("ordinal"))
        h, _ = self._readout_batch(batch, "saliency")
        gx = self.input_gradients(h, **kw)
        dev = next(iter(gx.values())).device if gx else None
        res = {}
        for t, g in gx.items():
            i = self.node_types.index(t)
            res[t] = self.saliency_scores(g, int(h.c.d_x[i]), int(h.c.ldx[i]), h.n_nodes[i], self.in_dims[t], groups, dev)
        return res

    def _salient_edge(self, edge_type, who: str) -> EdgeType:
        et = tuple(edge_type)
        if et not in self.edge_types:
            raise _lib.HydraMPError(f"{who}: the net has no edge type {et!r}")
        if self.in_dims.get(et[0], 0) <= 0:
            raise _lib.HydraMPError(f"{who}: node type '{et[0]}' has no input features to attribute to")
        return et

    def salient_edge_types(self) -> List[EdgeType]:
        """edge types of the live convs whose source type has input features (what the models' ``top_salient`` ranks by default)"""
        live = {c.edge_type for layer in self.layers for c in layer.convs if c.active}
        return [e for e in self.edge_types if e in live and self.in_dims.get(e[0], 0) > 0]

    def top_salient(self, batch, edge_type, k: int, out=None, passes=None, **kw):
        """``(src int64 [n_dst, k], score float32 [n_dst, k])`` on the device: for every destination row of ``edge_type`` the ``k``
        sources with the largest ``|gradient x input|``, descending, with the signed score; lower source index first on equal
        magnitude, a source reached by several edges once, ``-1`` / ``0`` past a row's sources (``top_attended``'s conventions;
        ``1 <= k <= 8``).  The scores are :meth:`saliency`'s ``gxi`` of the edge type's source type under ``**kw``
        (:meth:`input_gradients`' arguments): ONE gradient for all rows, i.e. what the selected outputs TOGETHER rest on.

        ``passes=P`` instead runs exact per-row passes: pass ``p < P`` explains output row ``ptr[g] + p`` of every graph ``g`` on
        its own (``ordinal=p``) and fills the destination rows of that ordinal only (the others keep what ``out`` held) -- the
        destination type must then be the head's output type.  All passes are queued without a host synchronisation.
        ``passes`` may also be a device int64 vector of output rows: one pass per listed row (a batch whose rows of interest are
        not its graphs' leading rows: the room nodes of a homogeneous batch).

        ``edge_type`` may also be a LIST of edge types: one gradient per pass serves them all and the result is
        ``{edge_type: (src, score)}`` (``out`` then a dict of pairs)."""
        who = "top_salient"
        k = _check_k(k)
        many = isinstance(edge_type, list)
        ets = [self._salient_edge(e, who) for e in (edge_type if many else [edge_type])]
        if passes is not None and (kw.get("rows") is not None or kw.get("ordinal") is not None):
            raise _lib.HydraMPError(f"{who}: passes and rows / ordinal overlap: per-row passes select their own rows")
        self._saliency_checks(who, kw.get("wrt", "logit"), kw.get("head", 0), kw.get("rows"), kw.get("ordinal"))
        head_t = self.head_type(int(kw.get("head", 0)))
        if passes is not None:
            for et in ets:
                if et[2] != head_t:
                    raise _lib.HydraMPError(f"{who}: per-row passes rank the sources of the output rows: edge type {et!r} does not end "
                                            f"in '{head_t}'")
        h, flat = self._readout_batch(batch, who)
        dev = flat.device
        idx = lambda t: self.node_types.index(t)  # noqa: E731
        res = {}
        for et in ets:
            if not h.c.d_x[idx(et[0])]:
                raise _lib.HydraMPError(f"{who}: the batch has no input features of node type '{et[0]}'")
            o = (out.get(et) if out is not None else None) if many else out
            if o is not None and (not isinstance(o, (tuple, list)) or len(o) != 2):
                raise _lib.HydraMPError(f"{who}: out must be a (src, score) pair of tensors")
            nd = h.n_nodes[idx(et[2])]
            res[et] = (_attention_buffer(o[0] if o is not None else None, nd, k, torch.int64, dev, "out[0]"),
                       _attention_buffer(o[1] if o is not None else None, nd, k, torch.float32, dev, "out[1]"), nd)
        gxi = {t: torch.empty(max(h.n_nodes[idx(t)], 1), dtype=torch.float32, device=dev) for t in {et[0] for et in ets}}
        plan = _lib.Plan()
        gbuf = {t: b for _, t, b, _ in self._gx_buffers(h, None, dev, who)}  # one set of gradient buffers for all passes
        if passes is None:
            todo = [(None, None, 0)]
        elif isinstance(passes, torch.Tensor):  # one pass per listed row r: ordinal 0 of the one-graph ptr [r, r + 1]
            if passes.dtype != torch.int64 or passes.dim() != 1 or passes.device != dev:
                raise _lib.HydraMPError(f"{who}: passes must be a pass count or an int64 vector of output rows on {dev}")
            ranges = torch.stack([passes, passes + 1], dim=1).contiguous()
            todo = [(0, ranges[r], 1) for r in range(ranges.size(0))]
        else:
            ptr, ng = self.graph_ptr(h, head_t, dev)
            todo = [(p, ptr, ng) for p in range(int(passes))]
        for p, ptr, ng in todo:
            g = self.input_gradients(h, out=gbuf, **(dict(kw, ordinal=(p, ptr) if isinstance(ptr, torch.Tensor) else p) if p is not None else kw))
            with torch.cuda.device(dev):
                for t, sc in gxi.items():
                    i = idx(t)
                    _lib.check(self._lib.hmp_saliency_scores(g[t].data_ptr(), int(h.c.ldx[i]), int(h.c.d_x[i]), int(h.c.ldx[i]),
                                                             h.n_nodes[i], self.in_dims[t], 0, None, None, sc.data_ptr(), None, None,
                                                             _lib.stream_ptr()))
                for et in ets:
                    _lib.check(self._lib.hmp_net_plan(self._handle, self.edge_types.index(et), C.byref(plan)))
                    _lib.check(self._lib.hmp_saliency_topk(plan, gxi[et[0]].data_ptr(), k, SEL_ORDINAL if p is not None else SEL_ALL, None,
                                                           p or 0, ptr.data_ptr() if p is not None else None, ng,
                                                           res[et][0].data_ptr(), res[et][1].data_ptr(), _lib.stream_ptr()))
        res = {et: (s_[:nd], w_[:nd]) for et, (s_, w_, nd) in res.items()}
        return res if many else res[ets[0]]

    def max_graph_rows(self, batch, node_type: str) -> int:
        """an upper bound of the ``node_type`` rows in one graph of the batch (the pass count of exact per-row explanations), from
        host-side numbers only: the collation's per-type maximum (``data.collate``, ``BatchStream.next``) or its largest graph where
        the batch is a union of graphs, else all rows (one graph)"""
        h, _ = self._readout_batch(batch, "max_graph_rows")
        i = self.node_types.index(node_type)
        if int(h.c.n_graphs) > 0 and h.c.d_node_ptr[i] and int(h.c.max_graph_nodes) > 0:
            return min(h.n_nodes[i], h.max_rows.get(i, int(h.c.max_graph_nodes)))
        return h.n_nodes[i]

    def explain_salient(self, batch, edge_type, k: int, passes: Optional[int] = None, **kw) -> Tuple[torch.Tensor, torch.Tensor]:
        """:meth:`top_salient` with exact per-row passes on the host: every pass lands in ONE device buffer (8 bytes per source,
        then 4 per score) that crosses in one D2H through one pinned buffer and one event, as :meth:`explain` moves its result.
        ``passes`` defaults to the largest output-row count of a graph of the batch.  Rows without a pass (none exist by default)
        hold ``-1`` / ``0``.  Returns host ``(src int64 [n_dst, k], score float32 [n_dst, k])``, views of that buffer (valid until
        the next call)."""
        k = _check_k(k)
        et = self._salient_edge(edge_type, "explain_salient")
        h, flat = self._readout_batch(batch, "explain_salient")
        dev = flat.device
        if passes is None:
            passes = self.max_graph_rows(h, et[2])
        nd = h.n_nodes[self.node_types.index(et[2])]
        n = nd * k
        with torch.cuda.device(dev):
            self._att.reserve(12 * n, dev)
            split = lambda buf: tuple(v.view(nd, k) for v in _pairs(buf, n))  # noqa: E731
            if n > 0:
                s_dev, w_dev = split(self._att.dev)
                s_dev.fill_(-1)
                w_dev.zero_()
                self.top_salient(h, et, k, out=(s_dev, w_dev), passes=passes, **kw)
            return split(self._att.fetch(12 * n))

    def _count(self, entry: str, h: _BatchHolder, dev, *args) -> None:
        """the count entries' common block: ``entry(handle, batch, *args, stream)`` (eval-mode forward + count on the device),
        which overwrites the activations of any earlier forward()"""
        with torch.cuda.device(dev):
            self._ensure_workspace(h, dev)
            _lib.check(getattr(self._lib, entry)(self._handle, C.byref(h.c), *args, _lib.stream_ptr()))
            self._fwd_token += 1
            self._plan_key = self._plan_tensors = None

    @property
    def n_classes(self) -> int:
        """width of the program's output (the class count of the room task)"""
        return int(self.layers[-1].out_dims[self.readout])

    def _forward_raw(self, h: _BatchHolder, training: bool, seed: int, rng_step: int) -> torch.Tensor:
        out_p, ld = C.c_void_p(), C.c_int32()
        _lib.check(self._lib.hmp_net_forward(self._handle, C.byref(h.c), self._flat.data_ptr(), int(training), seed, rng_step,
                                             C.byref(out_p), C.byref(ld), _lib.stream_ptr()))
        self._fwd_token += 1
        self._plan_key = self._plan_tensors = None
        out = self._ws_view(out_p.value, int(h.c.n_out), ld.value).clone()
        if self.aux_readout is None:
            return out
        rows = C.c_int32()
        _lib.check(self._lib.hmp_net_aux_output(self._handle, C.byref(out_p), C.byref(ld), C.byref(rows)))
        return out, self._ws_view(out_p.value, rows.value, ld.value).clone()

    def _backward_raw(self, gout: Optional[torch.Tensor], gaux: Optional[torch.Tensor] = None, d_gx=None) -> torch.Tensor:
        """``d_gx``: the executor's table of input-gradient buffers (one slot per node type, None = not wanted), else None"""
        dev = (gout if gout is not None else gaux).device
        grads = torch.zeros(self.n_params + 4, dtype=torch.float32, device=dev)
        if self.aux_readout is None:
            _lib.check(self._lib.hmp_net_backward(self._handle, gout.data_ptr(), gout.stride(0), self._flat.data_ptr(),
                                                  grads.data_ptr(), d_gx, _lib.stream_ptr()))
        else:
            _lib.check(self._lib.hmp_net_backward2(self._handle, gout.data_ptr() if gout is not None else None,
                                                   gout.stride(0) if gout is not None else 0,
                                                   gaux.data_ptr() if gaux is not None else None,
                                                   gaux.stride(0) if gaux is not None else 0, self._flat.data_ptr(),
                                                   grads.data_ptr(), d_gx, _lib.stream_ptr()))
        return grads

    def hidden(self, layer: int, node_type: str) -> torch.Tensor:
        """Copy (fp32) of the stored output of ``layer`` (1-based) for ``node_type`` from the last forward (``hmp_net_hidden``;
        diagnosis / tests).  Dropped elements are ``-0.0``."""
        p, ld, rows, width, b16 = C.c_void_p(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(self._lib.hmp_net_hidden(self._handle, int(layer), self.node_types.index(node_type), C.byref(p), C.byref(ld),
                                            C.byref(rows), C.byref(width), C.byref(b16)))
        esz = 2 if b16.value else 4
        off = p.value - self._ws.data_ptr()
        raw = self._ws[off:off + rows.value * ld.value * esz].view(torch.bfloat16 if b16.value else torch.float32)
        return raw.view(rows.value, ld.value)[:, :width.value].to(torch.float32).clone()

    STATUS_BITS = {1: "an edge endpoint is out of range (the edge was dropped)", 2: "a label is out of range",
                   4: "an edge lies outside the rows of the graph its Batch.ptr slice belongs to (stale or wrong edge `ptr`)"}

    def check_status(self) -> None:
        """Raise if a kernel flagged bad input data since the net was created (sticky device status word; synchronises).  The
        training loop reads the loss every step (``base_training_job.py:216``), which is where :meth:`TrainStep.loss` calls this."""
        _, status = self.read_state()
        if status:
            what = "; ".join(msg for bit, msg in self.STATUS_BITS.items() if status & bit) or "unknown bit"
            raise _lib.HydraMPError(f"device status word = {status}: {what}")

    def read_state(self) -> Tuple[int, int]:
        step, status = C.c_int32(), C.c_int32()
        _lib.check(self._lib.hmp_net_read_state(self._handle, C.byref(step), C.byref(status), _lib.stream_ptr()))
        return step.value, status.value


def _label_buffers(out, rows: Sequence[int], pair: bool, dev) -> List[torch.Tensor]:
    """the int64 label outputs of ``predict_labels``: fresh ones, or the caller's ``out`` after its checks"""
    if out is None:
        return [torch.empty(max(n, 1), dtype=torch.int64, device=dev) for n in rows]
    outs = list(out) if pair and isinstance(out, (tuple, list)) else [out]
    if len(outs) != len(rows) or not all(isinstance(o, torch.Tensor) for o in outs):
        raise _lib.HydraMPError(f"out: {'a pair of tensors (one per head)' if pair else 'one tensor'} expected")
    for o, n in zip(outs, rows):
        if o.dtype != torch.int64 or not o.is_contiguous() or o.device != dev or o.dim() != 1 or o.numel() < n:
            raise _lib.HydraMPError(f"out must be contiguous 1-d int64 tensors on {dev} with at least {n} rows, got "
                                    f"{tuple(o.shape)} {o.dtype} on {o.device}")
    return outs


TOPK_MAX = 8  # csrc/kernels.h


def _check_k(k) -> int:
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= TOPK_MAX:
        raise _lib.HydraMPError(f"k must be an integer in [1, {TOPK_MAX}], got {k!r}")
    return k


def _topk_buffers(out, rows: Sequence[int], k: int, pair: bool, dev) -> List[Tuple[torch.Tensor, torch.Tensor]]:
    """the ``(labels int64 [rows, k], probs float32 [rows, k])`` outputs of ``predict_topk`` per head: fresh ones, or the caller's
    ``out`` after the checks ``_label_buffers`` makes (dtype, rows, k columns, contiguity, device)"""
    if out is None:
        return [(torch.empty((max(n, 1), k), dtype=torch.int64, device=dev), torch.empty((max(n, 1), k), dtype=torch.float32, device=dev))
                for n in rows]
    outs = list(out) if pair else [out]
    ok = len(outs) == len(rows) and all(isinstance(o, (tuple, list)) and len(o) == 2 and all(isinstance(t, torch.Tensor) for t in o)
                                        for o in outs)
    if not ok:
        raise _lib.HydraMPError(f"out: {'a pair of (labels, probs) pairs (one per head)' if pair else 'one (labels, probs) pair'} expected")
    for (lb, pb), n in zip(outs, rows):
        for t, dtype in ((lb, torch.int64), (pb, torch.float32)):
            if t.dtype != dtype or not t.is_contiguous() or t.device != dev or t.dim() != 2 or t.size(1) != k or t.size(0) < n:
                raise _lib.HydraMPError(f"out must be contiguous (int64, float32) tensors [rows >= {n}, {k}] on {dev}, got "
                                        f"{tuple(t.shape)} {t.dtype} on {t.device}")
    return [(lb, pb) for lb, pb in outs]


MC_MAX_SAMPLES = 4096  # csrc/kernels.h


def _check_samples(samples) -> int:
    if isinstance(samples, bool) or not isinstance(samples, int) or not 1 <= samples <= MC_MAX_SAMPLES:
        raise _lib.HydraMPError(f"samples must be an integer in [1, {MC_MAX_SAMPLES}], got {samples!r}")
    return samples


def _check_first_step(first_step, samples: int) -> int:
    """the dropout step of sample 0: samples t = 0 .. samples - 1 draw at the 32-bit step ``first_step + t``"""
    if isinstance(first_step, bool) or not isinstance(first_step, int) or first_step < 0 or first_step + samples > 2 ** 32:
        raise _lib.HydraMPError(f"first_step must be an integer with 0 <= first_step and first_step + samples <= 2**32, got {first_step!r} "
                                f"with samples = {samples}")
    return first_step


def _check_seed(seed) -> int:
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
        raise _lib.HydraMPError(f"seed must be an integer in [0, 2**64), got {seed!r}")
    return seed


def _mc_buffers(out, rows: Sequence[int], classes: Sequence[int], pair: bool, dev) -> List[Tuple[torch.Tensor, ...]]:
    """the ``(labels int64 [rows], mean_probs float32 [rows, C], std, entropy, mutual_info float32 [rows])`` outputs of ``predict_mc``
    per head: fresh ones, or the caller's ``out`` after the checks ``_topk_buffers`` makes (structure, dtype, rows, C columns,
    contiguity, device)"""
    if out is None:
        return [(torch.empty(max(n, 1), dtype=torch.int64, device=dev), torch.empty((max(n, 1), c), dtype=torch.float32, device=dev))
                + tuple(torch.empty(max(n, 1), dtype=torch.float32, device=dev) for _ in range(3)) for n, c in zip(rows, classes)]
    outs = list(out) if pair and isinstance(out, (tuple, list)) else [out]
    ok = len(outs) == len(rows) and all(isinstance(o, (tuple, list)) and len(o) == 5 and all(isinstance(t, torch.Tensor) for t in o)
                                        for o in outs)
    if not ok:
        what = "(labels, mean_probs, std, entropy, mutual_info)"
        raise _lib.HydraMPError(f"out: {'a pair of ' + what + ' tuples (one per head)' if pair else 'one ' + what + ' tuple'} expected")
    for o, n, c in zip(outs, rows, classes):
        for i, t in enumerate(o):
            dtype, dim = (torch.int64 if i == 0 else torch.float32), (2 if i == 1 else 1)
            if (t.dtype != dtype or not t.is_contiguous() or t.device != dev or t.dim() != dim or t.size(0) < n
                    or (i == 1 and t.size(1) != c)):
                raise _lib.HydraMPError(f"out must be contiguous tensors (int64 [rows], float32 [rows, {c}], 3 x float32 [rows]) with rows "
                                        f">= {n} on {dev}, got {tuple(t.shape)} {t.dtype} on {t.device} at position {i}")
    return [tuple(o) for o in outs]


def _attention_buffer(out, rows: int, cols: int, dtype, dev, what: str) -> torch.Tensor:
    """one ``[rows, cols]`` output of the attention export: a fresh tensor, or the caller's after the checks of ``_topk_buffers``"""
    if out is None:
        return torch.empty((max(rows, 1), cols), dtype=dtype, device=dev)
    if (not isinstance(out, torch.Tensor) or out.dtype != dtype or not out.is_contiguous() or out.device != dev or out.dim() != 2
            or out.size(1) != cols or out.size(0) < rows):
        got = f"{tuple(out.shape)} {out.dtype} on {out.device}" if isinstance(out, torch.Tensor) else repr(type(out))
        raise _lib.HydraMPError(f"{what} must be a contiguous {dtype} tensor [rows >= {rows}, {cols}] on {dev}, got {got}")
    return out


def _check_counts4(counts: torch.Tensor, dev) -> None:
    if counts.dtype != torch.int64 or counts.numel() < 4 or not counts.is_contiguous() or counts.device != dev:
        raise _lib.HydraMPError("counts must be a contiguous int64[4] tensor on the model's device")


def _head_targets(net: NativeNet, h: _BatchHolder, labels, masks) -> _lib.HeadTargets:
    """hmp_head_targets for (readout labels, aux labels) and optional (readout mask, aux mask); the tensors it points at are
    appended to ``h.keep`` (kept alive with the descriptor, and part of a captured graph's key)."""
    if net.aux_readout is None:
        raise _lib.HydraMPError("the two-head entries need a two-headed net (aux_readout)")
    if len(labels) != 2 or (masks is not None and len(masks) != 2):
        raise _lib.HydraMPError("labels / masks: one tensor per head, (readout, aux)")
    tg = _lib.HeadTargets()
    for i, t in enumerate(net.head_label_types()):
        n = h.n_nodes[net.node_types.index(t)]
        lab = labels[i]
        _require_cuda(lab, f"labels[{i}]")
        lab = lab.to(torch.int64).contiguous()
        if lab is not labels[i]:
            h.converted = True
        if lab.numel() != n:
            raise _lib.HydraMPError(f"labels[{i}]: {lab.numel()} labels for {n} '{t}' rows")
        h.keep.append(lab)
        tg.d_labels[i] = lab.data_ptr() if n > 0 else None
        m = None if masks is None else masks[i]
        if m is not None:
            _require_cuda(m, f"masks[{i}]")
            if m.dtype != torch.bool:
                raise _lib.HydraMPError(f"masks[{i}] must be a bool tensor")
            m = m.contiguous()
            if m is not masks[i]:
                h.converted = True
            if m.numel() != n:
                raise _lib.HydraMPError(f"masks[{i}]: {m.numel()} entries for {n} '{t}' rows")
            h.keep.append(m)
            tg.d_mask[i] = m.data_ptr() if n > 0 else None
    return tg


class _NetFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net: NativeNet, holder: _BatchHolder, training: bool, seed: int, rng_step: int, *params):
        out = net._forward_raw(holder, training, seed, rng_step)
        ctx.net, ctx.holder, ctx.token = net, holder, net._fwd_token
        return out

    @staticmethod
    def backward(ctx, gout, gaux=None):
        net = ctx.net
        if ctx.token != net._fwd_token:
            raise _lib.HydraMPError(
                "backward() after another forward() of the same model: the native executor keeps the "
                "activations of the LAST forward only (one forward, then its backward)"
            )
        if gout is not None:
            gout = gout.contiguous()
            if gout.stride(0) % 4 != 0 or gout.data_ptr() % 16 != 0:
                padded = torch.zeros(gout.size(0), ((gout.size(1) + 3) // 4) * 4, dtype=gout.dtype, device=gout.device)
                padded[:, : gout.size(1)] = gout
                gout = padded
        if gaux is not None:
            gaux = gaux.contiguous()  # staged by the executor (any row pitch)
        want_x = getattr(ctx.holder, "grad_inputs", None) or []
        if gout is None and gaux is None:
            return (None,) * (5 + len(net.params) + len(want_x))
        d_gx, gx = None, []
        if want_x:
            if net.heads is not None or net._compute_bf16:
                raise _lib.HydraMPError("an input of the batch requires a gradient: not supported for nets with learned linear heads or in "
                                        "bf16 compute mode")
            h = ctx.holder
            dev = (gout if gout is not None else gaux).device
            d_gx = (C.c_void_p * _lib.MAX_NODE_TYPES)()
            for i in want_x:  # storage with the pitch of x; a node type the program never reads keeps 0
                n, F = h.n_nodes[i], net.in_dims[net.node_types[i]]
                buf = torch.zeros((max(n, 1), int(h.c.ldx[i])), dtype=torch.float32, device=dev)
                d_gx[i] = buf.data_ptr()
                gx.append(buf[:n, :F])
        flat_g = net._backward_raw(gout, gaux, d_gx)
        grads = []
        for p, live in zip(net.params, net.param_active):
            if not live:
                grads.append(None)
                continue
            off = net.param_offsets[id(p)]
            grads.append(flat_g[off:off + p.numel()].view(p.shape))
        return (None, None, None, None, None, *grads, *gx)


class TrainStep:
    """The loop body of ``BaseTrainingJob.train`` (``base_training_job.py:202-216``) as native code:
    phase A = plan + forward + masked CE + backward, [all-reduce], phase B = Adam.

    Gradients are SUMS over valid labels; ``{loss_sum, count}`` ride in the tail of the same flat
    buffer, so one all-reduce(sum) of ``n_active + 2`` floats makes the N-rank update equal to the
    single-process full-batch update (count-weighted mean), and every rank applies the identical Adam.

    The step kinds below differ only in their native entries (phase A alone, phases A + B in one call) and the targets
    they pass; this class runs every kind's step.
    """

    ENTRIES = ("hmp_net_step_fwd_bwd", "hmp_net_step_fused")

    def __init__(self, net: NativeNet, lr: float, weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8,
                 ignored_label: int = 25, seed: int = 0, training: bool = True, use_graph: bool = True,
                 process_group=None, force_collective: bool = False, view=None, comm=None, broadcast_init: bool = True):
        self.net = net
        # comm: parallel.NativeComm -- the all-reduce is enqueued by the library on the executor's own stream (RCCL);
        # process_group (True = default group): the same collective through torch.distributed (its own stream + event waits)
        self.comm = comm
        # homogeneous models: callable that presents their `Data` through the hetero accessors the executor reads
        self.view = view
        # run the data-parallel launch structure (two graphs around one all-reduce) even with a single rank
        self.force_collective = bool(force_collective)
        self.args = _lib.TrainArgs(lr, betas[0], betas[1], eps, weight_decay, ignored_label, seed, int(training))
        self.use_graph = use_graph
        self.pg = process_group
        self._graphs = None
        self._key = None
        self._stream = None
        self.flat = net.flat_params()
        dev = self.flat.device
        n = net.n_params + 4
        self.m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.v = torch.zeros(n, dtype=torch.float32, device=dev)
        self.grads = torch.zeros(n, dtype=torch.float32, device=dev)
        # Adam's t (and the dropout draw number) belong to the optimiser state, like m / v (torch.optim.Adam keeps
        # state['step'] per optimiser): a second TrainStep on the same net starts at t = 1, and a workspace re-bind
        # (a larger batch arrived) leaves it alone
        self.step_ctr = torch.zeros(4, dtype=torch.int32, device=dev)
        self.args.d_step = self.step_ctr.data_ptr()
        self._holder = None
        self._class_w = _NO_CLASS_W  # set_class_weight: one device vector (or None) per head; the identity of the tuple is the key
        self._targets = ()  # the entries' arguments between the batch and the parameters: byref(targets) but for one head
        self._batch_key = None
        self._data_ref = None
        if broadcast_init and self._world() > 1:
            # every rank starts from rank 0's weights: identical seeds are not relied upon
            if self.comm is not None:
                self.comm.broadcast_(self.flat, net.n_params)
            else:
                from . import parallel

                parallel.broadcast_parameters(self.flat, group=None if self.pg is True else self.pg)

    def _world(self) -> int:
        if self.comm is not None:
            return self.comm.world
        if self.pg is None:
            return 1
        import torch.distributed as dist

        return dist.get_world_size(self.pg if self.pg is not True else None)

    def _all_reduce(self) -> None:
        if self.comm is not None:
            if self.comm.world > 1 or self.force_collective:
                self.comm.all_reduce_sum_(self.grads, self.net.n_active + 2)
            return
        if self._world() > 1 or self.force_collective:
            from . import parallel

            parallel.allreduce_flat(self.grads, self.net.n_active, group=None if self.pg is True else self.pg,
                                    force=self.force_collective)

    def set_class_weight(self, weight) -> None:
        """Class weights of the step's cross entropy, ``F.cross_entropy(..., weight=w)``: from the next step on the loss is
        ``sum(w[y] * nll) / sum(w[y])`` over the valid labels, and Adam divides the summed gradients by that sum of weights.
        ``weight``: a float32 device tensor or a sequence of floats with one entry per class; for a two-headed step a pair
        ``(w_rooms, w_objects)`` or a dict ``{"rooms": w, "objects": w}`` (a missing or None entry leaves that head unweighted);
        None restores the unweighted step bit for bit.  The step keeps the tensors alive.  No launch is added; captured graphs
        hold the pointers as kernel arguments and are re-captured."""
        from .models.utils import class_weight_tensor

        classes = self.net.head_classes()
        if weight is None:
            per_head = [None] * len(classes)
        elif isinstance(weight, dict):
            unknown = set(weight) - {"rooms", "objects", "room", "object"}
            if unknown or len(classes) != 2:
                raise _lib.HydraMPError(f"class_weight: a dict names the heads 'rooms' and 'objects' of a two-headed step (got "
                                        f"{sorted(weight)} for {len(classes)} head(s))")
            per_head = [weight.get("rooms", weight.get("room")), weight.get("objects", weight.get("object"))]
        elif len(classes) == 2:
            if isinstance(weight, torch.Tensor) or len(weight) != 2:
                raise _lib.HydraMPError("class_weight: a two-headed step takes a pair (w_rooms, w_objects) or a dict")
            per_head = list(weight)
        else:
            per_head = [weight]
        dev = self.flat.device
        names = ("class_weight",) if len(classes) == 1 else ("class_weight[rooms]", "class_weight[objects]")
        ws = tuple(None if w is None else class_weight_tensor(w, c, dev, nm) for w, c, nm in zip(per_head, classes, names))
        self._class_w = _NO_CLASS_W if all(w is None for w in ws) else ws
        self._destroy_graphs()
        self._key = None

    def _phase_a(self, h, st):
        net = self.net
        _lib.check(getattr(net._lib, self.ENTRIES[0])(net._handle, C.byref(h.c), *self._targets, self.flat.data_ptr(),
                                                      self.grads.data_ptr(), C.byref(self.args), st))

    def _phase_ab(self, h, st):
        """single rank: both phases in one native call (Adam may ride in the gradient un-pack kernel)"""
        net = self.net
        _lib.check(getattr(net._lib, self.ENTRIES[1])(net._handle, C.byref(h.c), *self._targets, self.flat.data_ptr(),
                                                      self.grads.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                                                      C.byref(self.args), st))

    def _phase_b(self, st):
        net = self.net
        _lib.check(net._lib.hmp_net_step_adam(net._handle, self.flat.data_ptr(), self.grads.data_ptr(), self.m.data_ptr(),
                                              self.v.data_ptr(), C.byref(self.args), st))

    def _eager(self, h) -> None:
        st = _lib.stream_ptr()
        if self._world() == 1 and not self.force_collective:
            self._phase_ab(h, st)
        else:
            self._phase_a(h, st)
            self._all_reduce()
            self._phase_b(st)

    def __call__(self, data, labels: torch.Tensor) -> None:
        self._step(data, None, (labels,), labels, None)

    def _step(self, data, tag, tensors, labels, make_targets) -> None:
        """one step on ``data`` with the batch's ``labels`` or the targets ``make_targets(holder)`` builds; ``tensors`` (labels,
        masks ...) and ``tag`` key the descriptor cache"""
        net = self.net
        if net.flat_params(full_check=False) is not self.flat:
            raise _lib.HydraMPError(f"model parameters were moved after {type(self).__name__} was created")
        # the descriptor (and targets) of an unchanged batch object is reused (hydra_gnn_amd.data.HeteroData stamps every
        # mutation; foreign containers are described afresh every step)
        stamp = getattr(data, "_mutation_stamp", None)
        key = None
        if stamp is not None:
            key = (id(data), stamp(), tag) + tuple([(id(t), t._version) if t is not None else None for t in tensors])
        if key is not None and key == self._batch_key:
            h = self._holder
        else:
            h = net.make_batch(self.view(data) if self.view is not None else data, labels)
            self._targets = () if make_targets is None else (C.byref(make_targets(h)),)
            self._batch_key = key if not h.converted else None
            self._data_ref = (data, tensors)  # keeps id() unique while the key is live
        self._holder = h
        if net._class_w is not self._class_w:  # the weights are the net's (every step form reads them there): make them this step's
            net.set_class_weights(self._class_w)
        dev = self.flat.device
        with torch.cuda.device(dev):
            net._ensure_workspace(h, dev)
            net._fwd_token += 1  # the step overwrites the activations of any earlier forward()
            net._plan_key = net._plan_tensors = None
            if not self.use_graph:
                self._eager(h)
                return
            # the captured graph holds the descriptor's pointers (labels and masks among them: h.keep)
            key = (tuple(h.n_nodes), tuple(h.n_edges), tuple(t.data_ptr() for t in h.keep), id(net._ws))
            if self._graphs is None or key != self._key:
                self._capture(h, key)
            ga, gb = self._graphs
            cur = torch.cuda.current_stream()
            self._stream.wait_stream(cur)
            with torch.cuda.stream(self._stream):
                st = _lib.stream_ptr()
                _lib.check(net._lib.hmp_graph_launch(ga, st))
                if gb is not None:  # data parallel: the all-reduce sits between the two captured phases
                    self._all_reduce()
                    _lib.check(net._lib.hmp_graph_launch(gb, st))
            cur.wait_stream(self._stream)

    def _capture(self, h, key) -> None:
        net = self.net
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=self.flat.device)
        self._destroy_graphs()
        torch.cuda.synchronize(self.flat.device)
        with torch.cuda.stream(self._stream):
            st = _lib.stream_ptr()
            ga, gb = C.c_void_p(), C.c_void_p()
            single = self._world() == 1 and not self.force_collective  # no collective between the phases: ONE graph per step
            _lib.check(net._lib.hmp_graph_begin(st))
            try:
                if single:
                    self._phase_ab(h, st)
                else:
                    self._phase_a(h, st)
            finally:
                _lib.check(net._lib.hmp_graph_end(st, C.byref(ga)))
            if single:
                gb = None
            else:
                _lib.check(net._lib.hmp_graph_begin(st))
                try:
                    self._phase_b(st)
                finally:
                    _lib.check(net._lib.hmp_graph_end(st, C.byref(gb)))
        self._graphs, self._key, self._holder = (ga, gb), key, h

    def _destroy_graphs(self) -> None:
        if self._graphs is not None:
            for g in self._graphs:
                if g is not None:
                    self.net._lib.hmp_graph_destroy(g)
            self._graphs = None

    def __del__(self):
        try:
            self._destroy_graphs()
        except Exception:
            pass

    def run(self, holder: _BatchHolder) -> None:
        """One training step on a batch that is already described (``store.BatchStream.next``): no per-tensor Python, no
        descriptor cache -- the path a data loader that lives on the device drives.  Eager launches."""
        if getattr(getattr(holder, "stream", None), "two_headed", False):
            raise _lib.HydraMPError("TrainStep.run: the batch comes from a two-headed stream (labels and masks of two heads); step it "
                                    "with the model's semisupervised_step().run")
        want = getattr(getattr(holder, "stream", None), "ignored_label", None)  # a stream of homogeneous graphs wrote it into the labels
        if want is not None and want != self.args.ignored_label:
            raise _lib.HydraMPError(f"TrainStep.run: the step's ignored_label is {self.args.ignored_label}, the stream wrote its labels "
                                    f"with ignored_label {want} outside room_mask")
        self._run(holder)

    def _run(self, holder: _BatchHolder) -> None:
        net = self.net
        if self.use_graph:
            raise _lib.HydraMPError("TrainStep.run steps a NEW batch every call: create the step with use_graph=False")
        net._fwd_token += 1
        net._plan_key = net._plan_tensors = None
        self._batch_key = None
        self._holder = holder
        if net._class_w is not self._class_w:
            net.set_class_weights(self._class_w)
        self._eager(holder)

    def set_lr(self, lr: float) -> None:
        """Follow a learning-rate scheduler (``StepLR`` in ``base_training_job.py:186-188``): takes effect with the next
        step.  Captured graphs carry the rate as a kernel argument and are re-captured."""
        if C.c_float(float(lr)).value != self.args.lr:
            self.args.lr = float(lr)
            self._destroy_graphs()
            self._key = None

    def steps_taken(self) -> int:
        """Adam's t after the last step (synchronises)."""
        return int(self.step_ctr[0].item())

    def loss(self) -> float:
        """mean CE over the valid labels of the last step (global when data parallel); with class weights the weight-normalised
        mean ``sum(w * nll) / sum(w)``.  Synchronises."""
        t = self.grads[self.net.n_active: self.net.n_active + 2].tolist()
        self.net.check_status()
        return t[0] / (t[1] if t[1] > 0.0 else 1.0)  # a sum of weights below 1 is a normaliser too; no valid label: 0


class TwoHeadTrainStep(TrainStep):
    """The loop body of ``SemiSupervisedTrainingJob.train`` (semisupervised_training_job.py:117-147) as native code: phase A =
    plan + forward + the model's tail (act, dropout) + masked CE of BOTH heads + backward (``hmp_net_step2_fwd_bwd``), [all-reduce],
    phase B = Adam -- the :class:`TrainStep` contract with ``hmp_head_targets`` in place of the batch's labels.

    ``step(data, labels=(y_readout, y_aux), masks=(m_readout, m_aux) | None)``; :meth:`loss` is the summed CE of both heads
    divided by the total count, the reference's ``loss.item()``.  The dropout masks are the autograd path's (same seed, draw number
    = the step counter), so a step equals ``net(batch)`` -> ``net.loss`` -> ``backward`` -> ``torch.optim.Adam``."""

    ENTRIES = ("hmp_net_step2_fwd_bwd", "hmp_net_step2_fused")

    def __init__(self, net: NativeNet, lr: float, weight_decay: float = 0.0, ignored_label: int = -100, **kw):
        if net.aux_readout is None:
            raise _lib.HydraMPError("TwoHeadTrainStep needs a two-headed net (aux_readout); use TrainStep")
        super().__init__(net, lr, weight_decay=weight_decay, ignored_label=ignored_label, **kw)

    def __call__(self, data, labels, masks=None) -> None:
        tensors = tuple(labels) + (tuple(masks) if masks is not None else ())
        self._step(data, masks is None, tensors, None, lambda h: _head_targets(self.net, h, labels, masks))

    def run(self, holder, mask: Optional[str] = "train_mask") -> None:
        """One step on a device-collated batch of a two-headed stream (``store.stream(model, batch_size).next(ids)``): what
        :meth:`TrainStep.run` does, with the stream's own targets under the mask called ``mask`` (None = every row).  The stream's
        buffers never move, so its ``hmp_head_targets`` / ``hmp_linear_head_targets`` are built once per mask name."""
        stream = getattr(holder, "stream", None)
        if stream is None:
            raise _lib.HydraMPError(f"{type(self).__name__}.run takes a batch from store.BatchStream.next; step a data batch with "
                                    "step(data, ...)")
        if stream.nat is not self.net:
            raise _lib.HydraMPError(f"{type(self).__name__}.run: the batch comes from a stream created for another model")
        self._targets = (stream.targets(mask),)
        self._run(holder)


def _linear_head_targets(net: NativeNet, h: _BatchHolder, labels, mask, members) -> _lib.LinearHeadTargets:
    """hmp_linear_head_targets for per-row ``labels``, an optional bool ``mask`` and the bool ``members`` (room rows, object rows
    or None = the complement of the room rows); the tensors it points at join ``h.keep`` (alive with the descriptor, part of a
    captured graph's key)."""
    if net.heads is None:
        raise _lib.HydraMPError("the linear-head entries need a net with linear heads")
    n = int(h.c.n_out)
    tg = _lib.LinearHeadTargets()
    _require_cuda(labels, "labels")
    lab = labels.to(torch.int64).contiguous()
    if lab is not labels:
        h.converted = True
    if lab.numel() != n:
        raise _lib.HydraMPError(f"labels: {lab.numel()} labels for {n} output rows")
    h.keep.append(lab)
    tg.d_labels = lab.data_ptr() if n > 0 else None

    def rows(m, what):
        _require_cuda(m, what)
        if m.dtype != torch.bool:
            raise _lib.HydraMPError(f"{what} must be a bool tensor")
        c = m.contiguous()
        if c is not m:
            h.converted = True
        if c.numel() != n:
            raise _lib.HydraMPError(f"{what}: {c.numel()} entries for {n} output rows")
        h.keep.append(c)
        return c.data_ptr() if n > 0 else None

    if mask is not None:
        tg.d_mask = rows(mask, "mask")
    if members[0] is None:
        raise _lib.HydraMPError("the room head's rows (room_mask) are required")
    tg.d_member[0] = rows(members[0], "room_mask")
    if members[1] is not None:
        tg.d_member[1] = rows(members[1], "object_mask")
    return tg


class LinearHeadTrainStep(TwoHeadTrainStep):
    """The loop body of ``SemiSupervisedTrainingJob.train`` for the homogeneous two-headed models (HomogeneousNetwork /
    HomogeneousNeuralTreeNetwork with ``output_dim_dict``): phase A = plan + forward + the model's tail (act, dropout) + the two
    learned linear heads + masked CE of both + backward (``hmp_net_step_heads_fwd_bwd``), [all-reduce], phase B = Adam over
    [0, n_active), the heads included -- :class:`TrainStep`'s eager / graph / collective machinery with
    ``hmp_linear_head_targets``.

    ``step(data, labels=None, mask=None)``: labels default to ``data.y``, the mask to ``data.train_mask``; the room head's rows are
    ``data.room_mask``, the object head's ``data.<object_attr>`` (H-tree: ``object_mask``) or, with ``object_attr`` None, the
    complement of the room rows (the baseline's ``~room_mask``, computed on the device by the head kernel)."""

    ENTRIES = ("hmp_net_step_heads_fwd_bwd", "hmp_net_step_heads_fused")

    def __init__(self, net: NativeNet, lr: float, weight_decay: float = 0.0, ignored_label: int = -100,
                 object_attr: Optional[str] = None, **kw):
        if net.heads is None:
            raise _lib.HydraMPError("LinearHeadTrainStep needs a net with linear heads")
        TrainStep.__init__(self, net, lr, weight_decay=weight_decay, ignored_label=ignored_label, **kw)
        self.object_attr = object_attr

    def __call__(self, data, labels=None, mask=None) -> None:
        labels = data.y if labels is None else labels
        mask = data.train_mask if mask is None else mask
        members = (data.room_mask, getattr(data, self.object_attr) if self.object_attr is not None else None)
        tensors = (labels, mask) + members
        self._step(data, None, tensors, None, lambda h: _linear_head_targets(self.net, h, labels, mask, members))
