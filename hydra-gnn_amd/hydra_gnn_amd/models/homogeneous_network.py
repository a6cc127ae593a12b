"""``HomogeneousNetwork`` -- drop-in for the reference's ``src/hydra_gnn/models/homogeneous_network.py:11-147`` on the
MI355X engine.

GraphSAGE / GAT / GAT_edge: a homogeneous graph is the one-node-type, one-edge-type case of the native program
(:class:`hydra_gnn_amd.engine.NativeNet`, one launch sequence per step).  GCN / GIN (+ BatchNorm) -- the Stanford3DSG
``baseline_GCN`` / ``baseline_GIN`` configurations, SURVEY.md 8(f) row 2 -- are composed op by op from the native operators
of :mod:`hydra_gnn_amd.ops` (their graphs have 2..27 nodes; the per-layer launches do not matter there).
"""
from __future__ import annotations

import contextlib

import torch
import torch.nn as nn

from .. import ops
from ..engine import LayerDesc, NativeNet
from .._lib import ACT_ELU, ACT_NONE, ACT_RELU, HydraMPError
from .heterogeneous_network import _NativeModule
from .utils import BatchNorm, build_conv_layer, build_GAT_conv_layers

_NODE = "node"
_EDGE = (_NODE, "to", _NODE)


class _HomoView:
    """Presents a homogeneous ``Data`` (x, edge_index, edge_attr) through the hetero accessors."""

    def __init__(self, data):
        self._d = data

    @property
    def x_dict(self):
        return {_NODE: self._d.x}

    @property
    def edge_index_dict(self):
        return {_EDGE: self._d.edge_index}

    @property
    def edge_attr_dict(self):
        ea = getattr(self._d, "edge_attr", None)
        return {} if ea is None else {_EDGE: ea}


class HomogeneousNetwork(_NativeModule):
    def __init__(
        self,
        input_dim,
        output_dim=None,
        output_dim_dict=None,
        conv_block="GCN",
        hidden_dim=None,
        num_layers=None,
        GAT_hidden_dims=None,
        GAT_heads=None,
        GAT_concats=None,
        dropout=0.25,
        **kwargs
    ):
        super().__init__()
        if conv_block not in ("GraphSAGE", "GAT", "GAT_edge", "GCN", "GIN"):
            raise NotImplementedError(f"conv_block {conv_block}")
        self.conv_block = conv_block
        self.op_path = conv_block in ("GCN", "GIN")
        if output_dim is None:  # two-headed task of the semi-supervised Stanford job (reference :57-63,99-120)
            assert output_dim_dict is not None
            self.classification_task = "all"
            output_dim = hidden_dim
        else:
            assert output_dim_dict is None
            self.classification_task = "room"
        gat = conv_block[:3] == "GAT"
        self.num_layers = num_layers if not gat else len(GAT_heads)
        self.dropout = dropout
        self.input_dim = input_dim
        all_task = self.classification_task == "all"
        gat_dims = (list(GAT_hidden_dims) if all_task else list(GAT_hidden_dims) + [output_dim]) if gat else None
        if conv_block == "GAT":
            self.convs = build_GAT_conv_layers(input_dim, gat_dims, GAT_heads, GAT_concats, dropout=dropout)
        elif conv_block == "GAT_edge":
            self.convs = build_GAT_conv_layers(input_dim, gat_dims, GAT_heads, GAT_concats,
                                               dropout=dropout, edge_dim=3, add_self_loop=True,
                                               fill_value=torch.zeros(3, dtype=torch.float64))
        else:
            dims = [input_dim] + [hidden_dim] * (self.num_layers - 1) + [output_dim]
            self.convs = nn.ModuleList(build_conv_layer(conv_block, dims[l], dims[l + 1]) for l in range(self.num_layers))
        if conv_block == "GIN":  # reference :93-97 (one per layer, the last one is never used)
            self.batch_norms = nn.ModuleList(BatchNorm(hidden_dim) for _ in range(self.num_layers))
        if self.classification_task == "all":  # reference :99-120
            n_room = output_dim_dict["rooms"] if "rooms" in output_dim_dict else output_dim_dict["room"]
            n_obj = output_dim_dict["objects"] if "objects" in output_dim_dict else output_dim_dict["object"]
            final_hidden = (gat_dims[-1] * GAT_heads[-1] if GAT_concats[-1] else gat_dims[-1]) if gat else hidden_dim
            self.post_mp_room = nn.Linear(final_hidden, n_room)
            self.post_mp_object = nn.Linear(final_hidden, n_obj)
        self._init_native()

    def _build_native(self) -> NativeNet:
        if self.op_path:
            raise HydraMPError(f"{self.conv_block} runs op by op (hydra_gnn_amd.ops); there is no fused program / train_step "
                               "for it: use loss.backward() and an optimiser as the reference's training loop does")
        gat = self.conv_block[:3] == "GAT"
        layers = []
        for l, conv in enumerate(self.convs):
            cd = conv.desc(_EDGE)
            width = cd.f_out * (conv.heads if gat and conv.concat else 1)
            last = l == self.num_layers - 1
            act = ACT_NONE if last else (ACT_ELU if gat else ACT_RELU)
            layers.append(LayerDesc([cd], {_NODE: width}, act, 0.0 if last else self.dropout))
        return NativeNet([_NODE], {_NODE: self.input_dim}, [_EDGE], layers, readout=_NODE, **self._head_kw())

    def _head_kw(self):
        """two-headed task: the tail (act, dropout) and the learned heads the fused step runs natively (reference :138-146)"""
        if self.classification_task != "all":
            return {}
        gat = self.conv_block[:3] == "GAT"
        return dict(tail=(ACT_ELU if gat else ACT_RELU, float(self.dropout)), heads=[self.post_mp_room, self.post_mp_object])

    _OBJECT_ATTR = None  # rows of the object head: None = ~room_mask (reference :147)

    def _check_two_head(self, what):
        if self.classification_task != "all":
            raise HydraMPError(f"{what}: the model has one output (build it with output_dim_dict for the two-headed task); use "
                               "train_step()")
        if self.op_path:
            raise HydraMPError(f"{what}: {self.conv_block} runs op by op; the fused two-head step covers GraphSAGE / GAT / GAT_edge")

    def semisupervised_step(self, lr, weight_decay=0.0, class_weight=None, **kw):
        """Fused native step of the two-headed task (``SemiSupervisedTrainingJob.train``'s loop body, homogeneous branch), see
        engine.LinearHeadTrainStep: ``step(data, labels=None, mask=None)`` with ``data.y`` / ``data.train_mask`` as defaults and
        the head rows from ``data.room_mask``.  The dropout seed is the module's, so the masks are the ones ``forward()`` draws at
        the same step number."""
        from ..engine import LinearHeadTrainStep

        self._check_two_head("semisupervised_step")
        kw.setdefault("seed", self._seed)
        step = LinearHeadTrainStep(self.native(), lr=lr, weight_decay=weight_decay, view=self._view, object_attr=self._OBJECT_ATTR,
                                   **kw)
        if class_weight is not None:  # a pair (w_rooms, w_objects) or a dict {"rooms": w, "objects": w}
            step.set_class_weight(class_weight)
        return step

    def count_correct(self, data, mask_name="test_mask", counts=None):
        """The per-batch arithmetic of ``SemiSupervisedTrainingJob.test`` (semisupervised_training_job.py:198-257): eval-mode
        forward, argmax of both heads, compared with ``data.y`` on the rows of ``data.<mask_name>``.  With ``counts`` (device
        int64[4]) {correct_room, total_room, correct_object, total_object} are ADDED to it without a sync; without, returns the
        four ints of this batch.  ``data`` may be a descriptor from a two-headed ``store.BatchStream.next``: labels, head rows and
        the mask called ``mask_name`` are then the stream's own."""
        from ..engine import _BatchHolder

        self._check_two_head("count_correct")
        net = self.native()
        acc = counts
        if acc is None:
            acc = torch.zeros(4, dtype=torch.int64, device=net.flat_params(full_check=False).device)
        if isinstance(data, _BatchHolder):
            net.count_correct_stream(data, mask_name, acc)
            return acc if counts is not None else [int(v) for v in acc.tolist()]
        net.count_correct_heads(self._view(data), data.y, getattr(data, mask_name), self._members(data), acc)
        return acc if counts is not None else [int(v) for v in acc.tolist()]

    def _view(self, data):
        return _HomoView(data)

    # ---- GCN / GIN: op-by-op native path ---------------------------------------------------------------------------------
    def _drop_stream(self, l: int) -> int:
        """RNG tensor id of the feature dropout after conv ``l`` (the native program numbers its layers from 0, node type 0)"""
        return 8 * l

    def _act_drop(self, x, l, bias=None, _mc=None):
        """activation (relu; elu for GAT) + dropout after layer ``l`` (reference :135-136,141-142); the keep-mask is tensor
        ``_drop_stream(l)`` of this call's RNG step.  ``_mc = (seed, rng_step)``: a Monte-Carlo dropout pass -- dropout draws at
        that site whatever the ``training`` flag says, and the module's own seed and step are not looked at"""
        p = self.dropout if (self.training or _mc is not None) else 0.0
        seed, rng_step = (self._seed, self._rng_step) if _mc is None else _mc
        gat = self.conv_block[:3] == "GAT"
        return ops.bias_act_drop(x, bias, relu=not gat, elu=gat, p=p, seed=seed, rng_step=rng_step, rng_stream=self._drop_stream(l))

    def _op_layers(self, x, plan, batch_norm=True, _mc=None):
        """reference :125-136 for conv_block GCN / GIN; ``batch_norm`` False = the H-tree variant's loop, which never
        applies ``batch_norms`` (homogeneous_neural_tree_network.py:86-94).  ``_mc``: as :meth:`_act_drop` takes it (the caller
        holds the module in eval mode, so BatchNorm reads its running statistics and updates nothing)."""
        if self.training:
            self._rng_step += 1
        L = self.num_layers
        for l, conv in enumerate(self.convs):
            last = l == L - 1
            if self.conv_block == "GCN":
                a = ops.gcn_propagate(ops.project(x, conv.lin.weight), plan)
                x = ops.bias_act_drop(a, conv.bias) if last else self._act_drop(a, l, conv.bias, _mc=_mc)
            else:
                a = ops.gin_propagate(ops.project(x, conv.nn[0].weight), plan, conv.eps)
                h = ops.bias_act_drop(a, conv.nn[0].bias, relu=True)
                y = ops.bias_act_drop(ops.project(h, conv.nn[2].weight), conv.nn[2].bias)
                if last:
                    x = y
                else:
                    if batch_norm:
                        bn = self.batch_norms[l].module
                        y = ops.batch_norm(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps, self.training)
                        if self.training:
                            bn.num_batches_tracked += 1
                    x = self._act_drop(y, l, _mc=_mc)
        return x

    def _op_heads(self, x, room_mask, object_mask, _mc=None):
        """reference :138-146"""
        if self.classification_task == "room":
            return x[room_mask, :]
        x = self._act_drop(x, self.num_layers - 1, _mc=_mc)
        head = lambda lin, rows: ops.bias_act_drop(ops.project(rows, lin.weight), lin.bias)
        return head(self.post_mp_room, x[room_mask, :]), head(self.post_mp_object, x[object_mask, :])

    def _op_states(self, data, _mc=None):
        """final states of every node on the op path (GCN / GIN), before the readout"""
        return self._op_layers(data.x, ops.GraphPlan(data.edge_index, data.x.size(0)), _mc=_mc)

    def count_correct_rooms(self, data, counts=None, confusion=None, ignored_label=25):
        """The per-batch arithmetic of ``BaseTrainingJob.test`` (base_training_job.py:269-313) for the room task: eval-mode
        forward, ``argmax(dim=1)`` of the room rows, compared with ``data.y[data.room_mask]`` where the label is not
        ``ignored_label``.  The native output has a row per node, so ``data.room_mask`` is the kernel's row filter (no
        compaction).  SAGE / GAT: ``hmp_net_count_correct_rooms``; GCN / GIN: the op-by-op forward, then
        ``ops.count_correct_rows``.  With ``counts`` (device int64[2]) {correct, total} are ADDED to it without a sync; without,
        returns the two ints of this batch.  ``confusion`` (device int64 [C, C]) receives ``[label, pred] += 1``.  ``data`` may be
        a descriptor from ``store.stream(model, B, label_type="node").next(ids)``, which brings the labels and the ``room_mask``
        rows."""
        from ..engine import _BatchHolder

        self._room_task("count_correct_rooms")
        acc = counts
        if isinstance(data, _BatchHolder):  # store.BatchStream.next: labels and room_mask rows are the stream's
            net = self.native()
            if acc is None:
                acc = torch.zeros(2, dtype=torch.int64, device=net.flat_params(full_check=False).device)
            net.count_correct_rooms(data, None, acc, ignored_label, confusion=confusion)
            return acc if counts is not None else [int(v) for v in acc.tolist()]
        if acc is None:
            acc = torch.zeros(2, dtype=torch.int64, device=data.x.device)
        if not self.op_path:
            self.native().count_correct_rooms(self._view(data), data.y, acc, ignored_label, members=data.room_mask,
                                              confusion=confusion)
        else:
            ops.count_correct_rows(self._eval_states(data), data.y, acc, ignored_label, members=data.room_mask, confusion=confusion)
        return acc if counts is not None else [int(v) for v in acc.tolist()]

    @contextlib.contextmanager
    def _eval_mode(self):
        """eval mode without autograd; the training flag is put back"""
        was = self.training
        self.train(False)
        try:
            with torch.no_grad():
                yield
        finally:
            if was:
                self.train(True)

    def _eval_states(self, data):
        """GCN / GIN: the final states of an eval-mode op-by-op forward"""
        with self._eval_mode():
            return self._op_states(data)

    def count_correct_rooms_per_graph(self, data, counts, ignored_label=25, graph_ptr=None):
        """:meth:`count_correct_rooms` per graph (``BaseTrainingJob.test_individual_graph``, base_training_job.py:315-339, for a
        whole batch): ADDS {correct, total} of the batch's graph ``g`` to ``counts[g]`` (device int64 ``[num_graphs, 2]``) with one
        forward and one count launch, and returns it without a sync.  A stream descriptor brings labels, ``room_mask`` rows and
        row offsets; a collated ``Data`` keeps no ``ptr``, so it needs ``graph_ptr`` (device int64 ``[num_graphs + 1]`` node
        offsets).  SAGE / GAT: ``hmp_net_count_correct_rooms_by_graph``; GCN / GIN: the op-by-op forward, then
        ``ops.count_correct_rows_by_graph``."""
        from ..engine import _BatchHolder

        self._room_task("count_correct_rooms_per_graph")
        if isinstance(data, _BatchHolder):
            return self.native().count_correct_rooms_by_graph(data, None, counts, ignored_label)
        if graph_ptr is None:
            raise HydraMPError("count_correct_rooms_per_graph: a homogeneous Data batch keeps no ptr: pass graph_ptr= (device int64 "
                               "[num_graphs + 1] node offsets)")
        if not self.op_path:
            return self.native().count_correct_rooms_by_graph(self._view(data), data.y, counts, ignored_label, members=data.room_mask,
                                                              graph_ptr=graph_ptr)
        return ops.count_correct_rows_by_graph(self._eval_states(data), data.y, counts, graph_ptr, ignored_label,
                                               members=data.room_mask)

    def _object_rows(self, data):
        """rows of the object head, or None for the complement of ``room_mask`` (reference :147)"""
        return getattr(data, self._OBJECT_ATTR) if self._OBJECT_ATTR is not None else None

    def _members(self, data):
        """the row filter of the native label calls: ``room_mask``; two-headed: (room rows, object rows | None)"""
        return (data.room_mask, self._object_rows(data)) if self.classification_task == "all" else data.room_mask

    def _eval_heads(self, data):
        """GCN / GIN: both heads' logits of an eval-mode op-by-op forward"""
        with self._eval_mode():
            return self(data)

    def _scatter_heads(self, data, outs, per_head):
        """GCN / GIN, two-headed: the tensors ``per_head(logits)`` of each head scattered to the head's rows of its per-node buffers
        ``outs[head]``, ``-1`` (labels) / ``0`` (probabilities) elsewhere"""
        n = data.x.size(0)
        obj = self._object_rows(data)
        for bufs, logits, rows in zip(outs, self._eval_heads(data), (data.room_mask, ~data.room_mask if obj is None else obj)):
            for buf, values in zip(bufs, per_head(logits)):
                buf[:n].fill_(0 if buf.is_floating_point() else -1)
                buf[:n][rows] = values

    def predict_labels(self, data, out=None):
        """Labels on the device, one int64 per NODE (the native output has a row per node; nothing is compacted): room task:
        the room label on the rows of ``data.room_mask``, ``-1`` elsewhere; two-headed: a pair ``(room, object)`` of such vectors,
        ``-1`` outside ``room_mask`` and outside the object head's rows (``~room_mask``; H-tree: ``object_mask``).  ``data`` may be
        a descriptor from ``store.BatchStream.next``, which brings those rows.  SAGE / GAT: eval-mode native forward plus one launch
        (:meth:`NativeNet.predict_labels`), nothing synchronises.  GCN / GIN: the op-by-op eval forward, then
        ``hmp_predict_rows`` (room task) or ``hmp_argmax_rows`` per head scattered to the head's rows (two-headed) -- this path may
        synchronise inside torch (boolean row selection), as its ``forward()`` does."""
        from .._lib import require_device
        from ..engine import _BatchHolder

        require_device()  # no device: HydraMPError (there is no CPU fallback)
        two = self.classification_task == "all"
        if isinstance(data, _BatchHolder):
            if self.op_path:
                raise HydraMPError(f"predict_labels: {self.conv_block} runs op by op: pass a collated Data batch")
            return self.native().predict_labels(data, out=out)
        if not self.op_path:
            return self.native().predict_labels(self._view(data), out=out, members=self._members(data))
        if not two:
            return ops.predict_rows(self._eval_states(data), data.room_mask, out)
        from ..engine import _label_buffers

        n = data.x.size(0)
        outs = _label_buffers(out, [n, n], True, data.x.device)
        self._scatter_heads(data, [(o,) for o in outs], lambda logits: (ops.argmax_rows(logits),))
        return outs[0][:n], outs[1][:n]

    def predict_topk(self, data, k=1, out=None):
        """Top-k labels with their softmax probabilities on the device, one row per NODE as :meth:`predict_labels` lays them out:
        per head ``(labels [nodes, k] int64, probs [nodes, k] float32)``, ``labels[:, 0]`` its result, ``-1`` / ``0`` in all k
        columns outside the head's rows and in the columns past the class count.  Room task: ``(labels, probs)``; two-headed:
        ``((room_labels, room_probs), (object_labels, object_probs))``.  ``1 <= k <= 8``; ``data`` and ``out`` as
        :meth:`predict_labels` takes them (``out`` in that structure: contiguous, k columns).  SAGE / GAT: eval-mode native forward
        plus one launch (:meth:`NativeNet.predict_topk`).  GCN / GIN: the op-by-op eval forward, then ``hmp_topk_rows`` (two-headed:
        per head, scattered to the head's rows)."""
        from .._lib import require_device
        from ..engine import _BatchHolder, _check_k, _topk_buffers

        require_device()  # no device: HydraMPError (there is no CPU fallback)
        k = _check_k(k)
        two = self.classification_task == "all"
        if isinstance(data, _BatchHolder):
            if self.op_path:
                raise HydraMPError(f"predict_topk: {self.conv_block} runs op by op: pass a collated Data batch")
            return self.native().predict_topk(data, k, out=out)
        if not self.op_path:
            return self.native().predict_topk(self._view(data), k, out=out, members=self._members(data))
        if not two:
            return ops.topk_rows(self._eval_states(data), k, data.room_mask, out)
        n = data.x.size(0)
        outs = _topk_buffers(out, [n, n], k, True, data.x.device)
        self._scatter_heads(data, outs, lambda logits: ops.topk_rows(logits, k))
        return tuple((lb[:n], pb[:n]) for lb, pb in outs)

    def predict_with_confidence(self, data):
        """``(labels, confidence)`` on the host: :meth:`predict`'s labels (the ``room_mask`` rows; two-headed: each head's rows, in
        row order) and the softmax probability of each, column 0 of :meth:`predict_topk` with ``k = 1``, through one pinned buffer
        and one device-to-host copy (GCN / GIN: one copy per output).  A two-headed model returns a pair of those."""
        from .._lib import require_device

        require_device()  # no device: HydraMPError (there is no CPU fallback)
        two = self.classification_task == "all"
        if self.op_path:
            heads = self.predict_topk(data, 1)
            heads = [tuple(t[:, 0].cpu() for t in hd) for hd in (heads if two else (heads,))]
        else:
            heads = self.native().predict_confidence(self._view(data), members=self._members(data))
            heads = heads if two else (heads,)
        heads = tuple((lb[lb >= 0], pb[lb >= 0]) for lb, pb in heads)  # the rows outside a head's rows dropped on the host
        return heads if two else heads[0]

    def predict_mc(self, data, samples=16, seed=None, first_step=1, out=None):
        """Monte-Carlo dropout uncertainty on the device, one row per NODE as :meth:`predict_labels` lays them out: per head
        ``(labels int64 [nodes], mean_probs float32 [nodes, C], std, entropy, mutual_info float32 [nodes])`` over ``samples``
        stochastic passes, pass ``t`` drawing its dropout masks at ``(seed, first_step + t)`` (``seed`` None: the module's), ``-1`` /
        ``0`` outside the head's rows.  Room task: one such tuple; two-headed: a pair.  ``data`` and ``out`` as :meth:`predict_topk`
        takes them (``out`` in that structure).  SAGE / GAT: per pass the native training-mode forward plus one launch, then one
        launch per head (:meth:`NativeNet.predict_mc`).  GCN / GIN: per pass the op-by-op forward with dropout drawing and
        BatchNorm in eval mode (running statistics, nothing updated), then ``hmp_mc_accumulate_rows`` per head, and
        ``hmp_mc_finish`` (two-headed: scattered to the head's rows).  ``_rng_step``, the ``training`` flag, parameters and buffers
        are left as they were."""
        from .._lib import require_device
        from ..engine import _BatchHolder, _mc_buffers

        samples, seed, first_step = self._mc_args(samples, seed, first_step)
        require_device()  # no device: HydraMPError (there is no CPU fallback)
        two = self.classification_task == "all"
        if isinstance(data, _BatchHolder):
            if self.op_path:
                raise HydraMPError(f"predict_mc: {self.conv_block} runs op by op: pass a collated Data batch")
            with torch.no_grad():
                return self.native().predict_mc(data, samples, seed, first_step, out=out)
        if not self.op_path:
            with torch.no_grad():
                return self.native().predict_mc(self._view(data), samples, seed, first_step, members=self._members(data), out=out)
        n, dev = data.x.size(0), data.x.device
        if not two:
            classes = [int(self.convs[-1].lin.weight.size(0) if self.conv_block == "GCN" else self.convs[-1].nn[2].weight.size(0))]
        else:
            classes = [int(self.post_mp_room.out_features), int(self.post_mp_object.out_features)]
        outs = _mc_buffers(out, [n] * len(classes), classes, two, dev)
        obj = self._object_rows(data)
        head_rows = (data.room_mask, ~data.room_mask if obj is None else obj)
        accs = None
        with self._eval_mode():
            for t in range(samples):
                mc = (seed, first_step + t)
                states = self._op_states(data, _mc=mc)
                if not two:
                    accs = accs or [ops.mc_acc(n, classes[0], dev)]
                    ops.mc_accumulate_rows(states, accs[0], t == 0, data.room_mask)
                    continue
                logits = self._op_heads(states, head_rows[0], head_rows[1], _mc=mc)
                accs = accs or [ops.mc_acc(lg.size(0), c, dev) for lg, c in zip(logits, classes)]
                for lg, acc in zip(logits, accs):
                    ops.mc_accumulate_rows(lg, acc, t == 0)
            if not two:
                return ops.mc_finish(accs[0], classes[0], samples, data.room_mask, outs[0])
            for bufs, acc, c, rows in zip(outs, accs, classes, head_rows):
                for buf, values in zip(bufs, ops.mc_finish(acc, c, samples)):
                    buf[:n].fill_(0 if buf.is_floating_point() else -1)
                    buf[:n][rows] = values
        return tuple(tuple(b[:n] for b in bufs) for bufs in outs)

    def predict_with_uncertainty(self, data, samples=16):
        """``(labels, confidence, std, entropy, mutual_info)`` on the host: :meth:`predict_mc` with the module's seed on the head's
        rows (the ``room_mask`` rows; two-headed: each head's rows, in row order), ``confidence`` the mean probability of the label,
        through one pinned buffer and one device-to-host copy (GCN / GIN: one copy per output).  A two-headed model returns a pair
        of those."""
        from .._lib import require_device
        from .heterogeneous_network import _uncertainty_rows

        samples, seed, first_step = self._mc_args(samples, None, 1)
        require_device()  # no device: HydraMPError (there is no CPU fallback)
        if self.op_path:
            heads = self.predict_mc(data, samples)
            two = self.classification_task == "all"
            heads = tuple(tuple(t.cpu() for t in hd) for hd in (heads if two else (heads,)))
            return _uncertainty_rows(heads if two else heads[0])
        with torch.no_grad():
            heads = self.native().predict_uncertainty(self._view(data), samples, seed, first_step, members=self._members(data))
        return _uncertainty_rows(heads)

    def _predict_two(self, data):
        """host ``(room_labels, object_labels)``: the labels of the ``room_mask`` rows and of the object head's rows, in row order
        (the -1 rows of :meth:`predict_labels` dropped on the host)"""
        if self.op_path:
            return tuple(ops.argmax_rows(p).cpu() for p in self._eval_heads(data))
        pair = self.native().predict_pair(self._view(data), members=self._members(data))
        return tuple(p[p >= 0] for p in pair)

    def predict(self, data):
        """Room labels of ``data.room_mask``'s rows on the host (``GnnModel.infer``); a two-headed model returns host int64
        ``(room_labels, object_labels)`` = ``tuple(p.argmax(dim=1).cpu() for p in self(data))`` in eval mode."""
        if self.classification_task != "room":
            return self._predict_two(data)
        if not self.op_path:
            return super().predict(data)
        with torch.no_grad():
            return ops.argmax_rows(self(data)).cpu()

    _EXPLAIN_EDGE = _EDGE  # (H-tree: the LeafPool's edges, whose sources are the room's leaves)

    def explain_rooms(self, data, k=3, target=None, wrt="logit"):
        """Which nodes a room's label rests on, on the host: for every row of ``data.room_mask``, in row order, the ``k`` neighbours
        (sources of the room's incoming edges; H-tree model: the leaves of its LeafPool) with the largest ``|gradient x input|`` of the room's own predicted-class logit and
        their signed scores -- ``(nodes int64 [rooms, k], score float32 [rooms, k])``, ``-1`` / ``0`` past a room's neighbours.
        One exact pass per room (:meth:`NativeNet.top_salient` with the room rows as ``passes``): a collated homogeneous batch
        carries no graph offsets, and its rooms are not its graphs' leading rows.  The room rows are read from ``room_mask`` once
        up front; the passes are then queued without a synchronisation and the result crosses in one copy.  Room task, GraphSAGE /
        GAT / GAT_edge; ``target`` has one entry per NODE."""
        if self.classification_task != "room":
            raise HydraMPError("explain_rooms: the model is two-headed (learned linear heads): no input-gradient path")
        net = self._saliency_net("explain_rooms")
        rows = torch.nonzero(data.room_mask).flatten()  # (synchronises: the number of passes is a host number)
        src, score = net.explain_salient(self._view(data), self._EXPLAIN_EDGE, k, passes=rows, target=target, wrt=wrt)
        idx = rows.cpu()
        return src[idx], score[idx]

    def forward(self, data):
        if self.op_path:
            return self._op_heads(self._op_states(data), data.room_mask, ~data.room_mask)
        out = self._run(_HomoView(data))
        out = out[:, : self.native().layers[-1].out_dims[_NODE]]
        return self._op_heads(out, data.room_mask, ~data.room_mask)
