"""``HeterogeneousNetwork`` -- drop-in for the reference's
``src/hydra_gnn/models/heterogeneous_network.py:13-136`` on the MI355X engine.

Constructor signature, ``forward(data)``, ``loss(pred, label, mask)`` and the ``state_dict`` keys
(``convs.{layer}.convs.{src}__{rel}__{dst}.lin_l.weight`` ...) are the reference's.  ``forward`` runs the
whole layer stack natively (``hmp_net_forward``), the backward of ``loss.backward()`` runs
``hmp_net_backward``; there is no PyG / ATen message-passing path and no CPU fallback.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..data import EDGE_TYPES
from ..engine import LayerDesc, NativeNet
from .. import _lib
from .._lib import ACT_ELU, ACT_NONE, ACT_RELU
from .utils import build_GAT_hetero_conv, build_hetero_conv, cross_entropy_loss


def _uncertainty_rows(heads):
    """host ``predict_mc`` tuples (one, or a pair) as ``(labels, confidence, std, entropy, mutual_info)`` on the head's rows only:
    the rows outside a head's rows (label -1) dropped, ``confidence`` = the mean probability of the label"""
    two = isinstance(heads[0], tuple)
    out = []
    for lab, mean, sd, ent, mi in (heads if two else (heads,)):
        keep = lab >= 0
        lab = lab[keep]
        conf = mean[keep].gather(1, lab.view(-1, 1)).view(-1) if lab.numel() else mean.new_zeros(0)
        out.append((lab, conf, sd[keep], ent[keep], mi[keep]))
    return tuple(out) if two else out[0]


class _NativeModule(nn.Module):
    """Shared plumbing: lazily built :class:`NativeNet`, dropout RNG bookkeeping."""

    def _init_native(self):
        self._native = None
        self._rng_step = 0
        # drawn from torch's default generator so torch.manual_seed() controls the dropout stream
        self._seed = int(torch.randint(0, 2 ** 62, (1,)).item())

    def native(self) -> NativeNet:
        if self._native is None:
            self._native = self._build_native()
        return self._native

    def _run(self, data) -> torch.Tensor:
        net = self.native()
        if self.training:
            self._rng_step += 1
        return net.forward(data, self.training, self._seed, self._rng_step)

    def _drop_stream(self, l: int, node_type: str) -> int:
        """RNG tensor id of the feature dropout after conv ``l`` on ``node_type`` (executor numbering: 8 * program layer + node
        type index; a ``pre_mp`` layer in front shifts the program layers by one)"""
        net = self.native()
        return (l + len(net.layers) - self.num_layers) * 8 + net.node_types.index(node_type)

    def _tail_act_drop(self, x, stream: int):
        """activation + dropout on a final state of the two-headed task (reference heterogeneous_network.py:124-134): the native
        program ends at the last conv, this is ``hmp_bias_act_drop_*`` on its output; keep-mask = tensor ``stream`` of this call's
        RNG step (layer L-1 of the executor's numbering, which the executor itself never draws: its last layer has no dropout)"""
        from .. import ops

        gat = self.conv_block[:3] == "GAT"
        return ops.bias_act_drop(x, None, relu=not gat, elu=gat, p=self.dropout if self.training else 0.0, seed=self._seed,
                                 rng_step=self._rng_step, rng_stream=stream)

    def train_step(self, lr, weight_decay=0.0, class_weight=None, **kw):
        """Fused native training step (fwd + masked CE + bwd [+ all-reduce] + Adam), see engine.TrainStep.  ``class_weight``:
        the class weights of the cross entropy (``TrainStep.set_class_weight``), None = unweighted."""
        from ..engine import TrainStep

        if getattr(self, "classification_task", "room") != "room":
            raise NotImplementedError("the fused training step computes ONE masked cross entropy (room labels); the two-headed "
                                      "task has its own fused step: semisupervised_step()")
        step = TrainStep(self.native(), lr=lr, weight_decay=weight_decay, view=getattr(self, "_view", None), **kw)
        if class_weight is not None:
            step.set_class_weight(class_weight)
        return step

    def predict(self, data):
        """Room labels of ``data`` on the host: ``self(data).argmax(dim=1).cpu()`` as ``GnnModel.infer`` computes it
        (bin/room_classification_server:285-286), through the native inference path (:meth:`NativeNet.predict`).
        A two-headed model returns host int64 ``(room_labels, object_labels)`` =
        ``tuple(p.argmax(dim=1).cpu() for p in self(data))`` in eval mode, with one D2H for both (:meth:`NativeNet.predict_pair`)."""
        if getattr(self, "classification_task", "room") == "all":
            return self._predict_two(data)
        net = self.native()
        view = getattr(self, "_view", None)
        labels = net.predict(view(data) if view is not None else data, net.layers[-1].out_dims[net.readout])
        mask = getattr(data, "room_mask", None) if view is not None else None
        return labels if mask is None else labels[mask.cpu()]

    def _predict_two(self, data):
        """heterogeneous two-headed models: one label per ``rooms`` / ``objects`` row (H-tree: per ``room_virtual`` /
        ``object_virtual`` row)"""
        return self.native().predict_pair(data)

    def predict_labels(self, data, out=None):
        """The labels :meth:`predict` returns, left on the device (int64; nothing synchronises): eval-mode native forward plus one
        launch (:meth:`NativeNet.predict_labels`).  Room task: one label per output row; two-headed: a pair, one label per row of
        each head's label type.  ``data`` is a batch or a descriptor from ``store.BatchStream.next``; ``out`` takes caller-owned
        contiguous device int64 buffers (one, or a pair) of at least the needed rows."""
        _lib.require_device()  # no device: HydraMPError (there is no CPU fallback)
        return self.native().predict_labels(data, out=out)

    def predict_topk(self, data, k=1, out=None):
        """Top-k labels with their softmax probabilities, left on the device (nothing synchronises): eval-mode native forward plus
        one launch (:meth:`NativeNet.predict_topk`).  Per head ``(labels [rows, k] int64, probs [rows, k] float32)`` over the rows
        of :meth:`predict_labels` -- ``labels[:, 0]`` is its result, ``probs`` the softmax of what ``forward()`` returns in eval
        mode; columns past the class count hold ``-1`` / ``0``.  Room task: ``(labels, probs)``; two-headed:
        ``((room_labels, room_probs), (object_labels, object_probs))``.  ``1 <= k <= 8``; ``out`` takes caller-owned buffers of
        that structure (contiguous, k columns, at least the needed rows)."""
        _lib.require_device()  # no device: HydraMPError (there is no CPU fallback)
        return self.native().predict_topk(data, k, out=out)

    def predict_with_confidence(self, data):
        """``(labels, confidence)`` of ``data`` on the host: :meth:`predict`'s labels and the softmax probability of each (column 0
        of :meth:`predict_topk` with ``k = 1``), through one pinned buffer and one device-to-host copy.  A two-headed model returns
        a pair of those, ``((room_labels, room_confidence), (object_labels, object_confidence))``."""
        _lib.require_device()  # no device: HydraMPError (there is no CPU fallback)
        return self.native().predict_confidence(data)

    # ---- Monte-Carlo dropout uncertainty -------------------------------------------------------------------------------
    def _mc_args(self, samples, seed, first_step):
        """the checked ``(samples, seed, first_step)`` of a Monte-Carlo call; ``seed`` None: the module's dropout seed"""
        from ..engine import _check_first_step, _check_samples, _check_seed

        samples = _check_samples(samples)
        return samples, _check_seed(self._seed if seed is None else seed), _check_first_step(first_step, samples)

    def predict_mc(self, data, samples=16, seed=None, first_step=1, out=None):
        """Monte-Carlo dropout uncertainty, left on the device (nothing synchronises): ``samples`` stochastic passes -- pass ``t`` is
        the training-mode ``forward()`` with the dropout masks of ``(seed, first_step + t)`` -- reduced per row to
        ``(labels int64 [rows], mean_probs float32 [rows, C], std, entropy, mutual_info float32 [rows])`` over the rows of
        :meth:`predict_labels`: the mean softmax over the passes, its argmax, the standard deviation of that label's probability,
        the entropy of the mean and the mutual information between prediction and weights (BALD).  Room task: one such tuple;
        two-headed: a pair.  Each pass is the native training-mode forward plus one launch, one more launch per head finishes
        (:meth:`NativeNet.predict_mc`).  ``seed`` None: the module's dropout seed.  The module is left as it was: ``_rng_step`` is
        neither read nor advanced, the ``training`` flag, parameters and buffers are untouched.  ``1 <= samples <= 4096``; ``out``
        takes caller-owned buffers of that structure."""
        samples, seed, first_step = self._mc_args(samples, seed, first_step)
        _lib.require_device()  # no device: HydraMPError (there is no CPU fallback)
        with torch.no_grad():
            return self.native().predict_mc(data, samples, seed, first_step, out=out)

    def predict_with_uncertainty(self, data, samples=16):
        """``(labels, confidence, std, entropy, mutual_info)`` of ``data`` on the host: :meth:`predict_mc` with the module's seed,
        ``confidence`` being the mean probability of the label, through one pinned buffer and one device-to-host copy.  A two-headed
        model returns a pair of those."""
        samples, seed, first_step = self._mc_args(samples, None, 1)
        _lib.require_device()  # no device: HydraMPError (there is no CPU fallback)
        with torch.no_grad():
            heads = self.native().predict_uncertainty(data, samples, seed, first_step)
        return _uncertainty_rows(heads)

    # ---- attention export ([PyG] GATConv(..., return_attention_weights=True)) ----------------------------------------
    def _attention_layer(self, layer, who: str) -> int:
        """program layer of the model's conv layer ``layer`` (an int counting ``self.convs``, negative from the end) or of
        ``"pre_mp"``, the H-tree models' initialisation layer where it is a GAT layer of the native program"""
        if self.conv_block[:3] != "GAT":
            raise _lib.HydraMPError(f"{who}: no attention coefficients: conv_block {self.conv_block} has no attention (GAT and "
                                    "GAT_edge models export them)")
        first = len(self.native().layers) - self.num_layers  # 1 with pre_mp in front
        if layer == "pre_mp":
            if first == 0:
                raise _lib.HydraMPError(f"{who}: the model has no pre_mp layer (disable_initialization)")
            return 0
        if isinstance(layer, bool) or not isinstance(layer, int) or not -self.num_layers <= layer < self.num_layers:
            raise _lib.HydraMPError(f"{who}: layer must be 'pre_mp' or an int in [{-self.num_layers}, {self.num_layers}), got {layer!r}")
        return first + layer % self.num_layers

    def _attention_input(self, data):
        from ..engine import _BatchHolder

        view = getattr(self, "_view", None)
        return data if view is None or isinstance(data, _BatchHolder) else view(data)

    def attention(self, data, layer=-1):
        """Attention coefficients of conv layer ``layer`` (``-1``: the last; ``"pre_mp"``: the H-tree initialisation layer), left on
        the device (nothing synchronises): eval-mode native forward plus one launch (:meth:`NativeNet.attention`).  Heterogeneous
        models return ``{edge_type: alpha}`` for every conv whose output reaches the model's output, homogeneous models the one
        tensor.  ``alpha`` is float32 ``[E + n_loop, heads]`` in the order of ``hydra_gnn_amd.data.attention_edge_index(edge_index,
        n_loop)``: the input edges, then the self loops a same-type conv appends; an input self loop such a conv removes holds 0.
        ``data`` is a batch or a descriptor from ``store.BatchStream.next``."""
        l = self._attention_layer(layer, "attention")
        _lib.require_device()  # no device: HydraMPError (there is no CPU fallback)
        res = self.native().attention(self._attention_input(data), l)
        return next(iter(res.values())) if len(self.native().node_types) == 1 else res  # one node type: one conv per layer

    def top_attended(self, data, edge_type=None, k=3, layer=-1):
        """``(src int64 [n_dst, k], weight float32 [n_dst, k])`` on the device: per destination row of the conv on ``edge_type``
        in conv layer ``layer`` the ``k`` sources with the largest head-mean attention, descending (:meth:`NativeNet.top_attended`:
        eval-mode native forward plus one launch, nothing synchronises; ``1 <= k <= 8``; ``-1`` / ``0`` past a row's entries).
        Heterogeneous models: ``edge_type=None`` returns ``{edge_type: (src, weight)}`` for every conv :meth:`attention` exports;
        homogeneous models have one edge type per layer and return its pair."""
        l = self._attention_layer(layer, "top_attended")
        _lib.require_device()  # no device: HydraMPError (there is no CPU fallback)
        net = self.native()
        homog = len(net.node_types) == 1
        if edge_type is None:
            ets = net.attention_edge_types(l)
            return net.top_attended(self._attention_input(data), l, ets[0] if homog else ets, k)
        return net.top_attended(self._attention_input(data), l, tuple(edge_type), k)

    # ---- gradient saliency ([PyG] idiom: x.requires_grad_(); model(data)[i, c].backward(); x.grad) --------------------
    def _saliency_net(self, who: str) -> NativeNet:
        """the native net after the refusals that need no device, or HydraMPError without one"""
        if getattr(self, "op_path", False):
            raise _lib.HydraMPError(f"{who}: {self.conv_block} models run op by op (hydra_gnn_amd.ops), not the native program: they "
                                    "have no input-gradient path (GraphSAGE, GAT and GAT_edge models do)")
        net = self.native()
        net._saliency_checks(who, "logit", 0, None, None)
        _lib.require_device()  # no device: HydraMPError (there is no CPU fallback)
        return net

    def _saliency_rows(self, data, rows):
        """the default row selection: every output row; homogeneous room classifiers: the rows of ``room_mask`` (the native output
        has a row per node, the model's output the room rows)"""
        from ..engine import _BatchHolder

        if rows is not None or getattr(self, "_view", None) is None:
            return rows
        if isinstance(data, _BatchHolder):
            if data.stream is not None and getattr(data.stream, "homog_room", False):
                return data.stream.members[:int(data.c.n_out)]  # the collated room_mask of the current batch
            return None
        return getattr(data, "room_mask", None)

    def input_gradients(self, data, target=None, rows=None, wrt="logit", head=0, ordinal=None):
        """Gradient of the chosen class's logit (``wrt="logit"``) or log-probability (``"logprob"``), summed over the selected
        output rows, with respect to the input features, left on the device (nothing synchronises): eval-mode native forward, one
        seed launch and the backward chain without the weight gradients (:meth:`NativeNet.input_gradients`).  Heterogeneous
        models return ``{node_type: gx [n_t, F_t]}``, homogeneous models the one tensor.

        ``target``: int64 class per native output row (None: the row's prediction, :meth:`predict_labels`); ``rows``: bool
        selection of output rows (None: all; homogeneous models: ``data.room_mask``, and ``target`` / ``rows`` have one entry per
        NODE); ``ordinal=p``: the ``p``-th output row of every graph of the batch instead.  ``head=1``: the object head of a
        two-headed heterogeneous model.  ``data`` is a batch or a descriptor from ``store.BatchStream.next``."""
        net = self._saliency_net("input_gradients")
        res = net.input_gradients(self._attention_input(data), target=target, rows=self._saliency_rows(data, rows) if ordinal is None else None,
                                  ordinal=ordinal, wrt=wrt, head=head)
        return next(iter(res.values())) if len(net.node_types) == 1 else res

    def saliency(self, data, groups=((0, 3), (3, 6), (6, None)), target=None, rows=None, wrt="logit", head=0, ordinal=None):
        """Per node type ``(gxi [n], gnorm [n], groups [n, n_groups])`` on the device: :meth:`input_gradients` reduced against the
        input per node row (:meth:`NativeNet.saliency`): signed gradient x input, gradient norm, and gradient x input per column
        range of ``groups`` (at most 4 ``(lo, hi)``, ``hi`` None = the last column; the default splits the 306-d object features
        into position, box size and the word2vec block).  Heterogeneous models return ``{node_type: triple}``, homogeneous
        models the one triple.  Nothing synchronises."""
        net = self._saliency_net("saliency")
        res = net.saliency(self._attention_input(data), groups=groups, target=target,
                           rows=self._saliency_rows(data, rows) if ordinal is None else None, ordinal=ordinal, wrt=wrt, head=head)
        return next(iter(res.values())) if len(net.node_types) == 1 else res

    def top_salient(self, data, edge_type=None, k=3, target=None, rows=None, wrt="logit", head=0):
        """``(src int64 [n_dst, k], score float32 [n_dst, k])`` on the device: per destination row of ``edge_type`` the ``k``
        sources with the largest ``|gradient x input|`` under ONE gradient for all selected rows (:meth:`NativeNet.top_salient`;
        ``top_attended``'s conventions, the score signed).  Heterogeneous models: ``edge_type=None`` returns ``{edge_type: (src,
        score)}`` for every live conv whose source type has input features; homogeneous models return their one pair."""
        net = self._saliency_net("top_salient")
        homog = len(net.node_types) == 1
        kw = dict(target=target, rows=self._saliency_rows(data, rows), wrt=wrt, head=head)
        if edge_type is None:
            ets = net.salient_edge_types()
            return net.top_salient(self._attention_input(data), ets[0] if homog else ets, k, **kw)
        return net.top_salient(self._attention_input(data), tuple(edge_type), k, **kw)

    _EXPLAIN_EDGE = None  # the edge type whose sources explain_rooms ranks for every output row (None: the model has none)

    def _explain_by_gradient(self, data, k, target=None, wrt="logit"):
        """exact per-room passes in ordinal mode over the readout's ``ptr``, all queued into one output, one copy at the end"""
        if self._EXPLAIN_EDGE is None:
            raise _lib.HydraMPError(f"explain_rooms: {type(self).__name__} has no edge type that ends in its output rows to rank over "
                                    "(use top_salient / saliency)")
        if getattr(self, "classification_task", "room") != "room":
            raise _lib.HydraMPError("explain_rooms: the model is two-headed; use top_salient(head=...)")
        net = self._saliency_net("explain_rooms")
        return net.explain_salient(self._attention_input(data), self._EXPLAIN_EDGE, k, target=target, wrt=wrt)

    def loss(self, pred, label, mask=None, weight=None):
        return cross_entropy_loss(pred, label, mask, weight)

    _ROOM_LABELS = "rooms"  # node type whose `y` BaseTrainingJob.test compares with (base_training_job.py:283-291)

    def _room_task(self, what):
        if getattr(self, "classification_task", "room") != "room":
            raise _lib.HydraMPError(f"{what}: the model is two-headed (built with output_dim_dict); count its accuracy with "
                                    "count_correct()")

    def count_correct_rooms(self, data, counts=None, confusion=None, ignored_label=25):
        """The per-batch arithmetic of ``BaseTrainingJob.test`` (base_training_job.py:269-313) for the room task: eval-mode native
        forward, ``argmax(dim=1)``, compared with the room labels (``data["rooms"].y``, H-tree: ``data["room_virtual"].y``) on
        the rows whose label is not ``ignored_label`` (``hmp_net_count_correct_rooms``).  ``data`` is a batch or a descriptor from
        ``store.BatchStream.next`` (its labels come from the stream's ``label_type``).  With ``counts`` (device int64[2]) the
        batch's {correct, total} are ADDED to it on the device and the tensor is returned without a sync; without, returns the two
        ints of this batch.  ``confusion`` (device int64 [C, C]) receives ``[label, pred] += 1`` of the counted rows."""
        from ..engine import _BatchHolder

        self._room_task("count_correct_rooms")
        net = self.native()
        acc = counts
        if acc is None:
            acc = torch.zeros(2, dtype=torch.int64, device=net.flat_params(full_check=False).device)
        labels = None if isinstance(data, _BatchHolder) else data[self._ROOM_LABELS].y
        net.count_correct_rooms(data, labels, acc, ignored_label, confusion=confusion)
        return acc if counts is not None else [int(v) for v in acc.tolist()]

    def count_correct_rooms_per_graph(self, data, counts, ignored_label=25, graph_ptr=None):
        """:meth:`count_correct_rooms` per graph (``BaseTrainingJob.test_individual_graph``, base_training_job.py:315-339, for a
        whole batch): one eval-mode forward and one count launch (``hmp_net_count_correct_rooms_by_graph``) ADD {correct, total}
        of the batch's graph ``g`` to ``counts[g]`` (device int64 ``[num_graphs, 2]``), which is returned without a sync.  A stream
        descriptor brings labels and row offsets; a collated batch is read through ``ptr`` of the room labels' node type unless
        ``graph_ptr`` (device int64 ``[num_graphs + 1]``) is given."""
        from ..engine import _BatchHolder

        self._room_task("count_correct_rooms_per_graph")
        net = self.native()
        if isinstance(data, _BatchHolder):
            return net.count_correct_rooms_by_graph(data, None, counts, ignored_label)
        store = data[self._ROOM_LABELS]
        if graph_ptr is None:
            graph_ptr = getattr(store, "ptr", None)
            if graph_ptr is None:
                raise _lib.HydraMPError(f"count_correct_rooms_per_graph: the batch has no '{self._ROOM_LABELS}'.ptr (collate it, or pass "
                                        "graph_ptr=)")
        return net.count_correct_rooms_by_graph(data, store.y, counts, ignored_label, graph_ptr=graph_ptr)


def _hetero_layers(module, node_types):
    """LayerDesc list from ``module.convs`` (a ModuleList of HeteroConv containers)."""
    gat = module.conv_block[:3] == "GAT"
    layers = []
    L = module.num_layers
    for l, hc in enumerate(module.convs):
        convs = [hc.conv(et).desc(et) for et in hc.edge_types]
        out_dims = {}
        for et, cd in zip(hc.edge_types, convs):
            c = hc.conv(et)
            width = cd.f_out * (c.heads if gat and c.concat else 1)
            assert out_dims.setdefault(et[2], width) == width, "convs reaching one node type must agree on the width"
        last = l == L - 1
        act = ACT_NONE if last else (ACT_ELU if gat else ACT_RELU)
        layers.append(LayerDesc(convs, out_dims, act, 0.0 if last else module.dropout, group_mean=(hc.aggr == "mean")))
    return layers


class _HeteroTwoHead(_NativeModule):
    """The two-headed task's native entries, shared by the heterogeneous models built with ``output_dim_dict``
    (HeterogeneousNetwork: the final states; HeterogeneousNeuralTreeNetwork: their LeafPool, ``NativeNet.head_pools``)."""

    def semisupervised_step(self, lr, weight_decay=0.0, class_weight=None, **kw):
        """Fused native step of the two-headed task (``SemiSupervisedTrainingJob.train``'s loop body), see
        engine.TwoHeadTrainStep: ``step(data, labels=(y_rooms, y_objects), masks=(m_rooms, m_objects))``.  The dropout seed is
        the module's, so the masks are the ones ``forward()`` draws at the same step number.  HeterogeneousNeuralTreeNetwork:
        labels and masks of the pooled rows, ``(room_virtual, object_virtual)``."""
        from ..engine import TwoHeadTrainStep

        if getattr(self, "classification_task", "room") != "all":
            raise _lib.HydraMPError("semisupervised_step: the model has one output (build it with output_dim_dict for the "
                                    "two-headed task); use train_step()")
        kw.setdefault("seed", self._seed)
        step = TwoHeadTrainStep(self.native(), lr=lr, weight_decay=weight_decay, **kw)
        if class_weight is not None:  # a pair (w_rooms, w_objects) or a dict {"rooms": w, "objects": w}
            step.set_class_weight(class_weight)
        return step

    def count_correct(self, data, labels=None, masks=None, counts=None):
        """The per-batch arithmetic of ``SemiSupervisedTrainingJob.test`` (semisupervised_training_job.py:198-257): eval-mode
        forward, argmax of both heads, compared with ``labels = (y_rooms, y_objects)`` under ``masks``.  With ``counts`` (device
        int64[4]) the batch's {correct_rooms, total_rooms, correct_objects, total_objects} are ADDED to it on the device and the
        tensor is returned without a sync (a loader loop reads it once per pass); without, returns the four ints of this batch.
        The H-tree model's heads are its pooled rows: labels and masks of ``room_virtual`` / ``object_virtual``.
        ``data`` may be a descriptor from a two-headed ``store.BatchStream.next``: the labels are the stream's (pass none) and
        ``masks`` is the NAME of the mask (``"train_mask"`` / ``"val_mask"`` / ``"test_mask"``; None = every row)."""
        from ..engine import _BatchHolder

        net = self.native()
        if net.aux_readout is None:
            raise _lib.HydraMPError("count_correct: the model has one output (build it with output_dim_dict)")
        acc = counts
        if acc is None:
            acc = torch.zeros(4, dtype=torch.int64, device=net.flat_params(full_check=False).device)
        if isinstance(data, _BatchHolder):
            if labels is not None or not (masks is None or isinstance(masks, str)):
                raise _lib.HydraMPError("count_correct: a stream batch brings its own labels (pass labels=None) and takes the mask by "
                                        "name (masks='val_mask')")
            net.count_correct_stream(data, masks, acc)
        else:
            if labels is None:
                raise _lib.HydraMPError("count_correct: labels are required for a data batch")
            net.count_correct(data, labels, masks, acc)
        return acc if counts is not None else [int(v) for v in acc.tolist()]


class HeterogeneousNetwork(_HeteroTwoHead):
    def __init__(
        self,
        input_dim_dict,
        output_dim=None,
        output_dim_dict=None,
        conv_block="GraphSAGE",
        hidden_dim=None,
        num_layers=None,
        GAT_hidden_dims=None,
        GAT_heads=None,
        GAT_concats=None,
        dropout=0.25,
        **kwargs
    ):
        """Arguments as in the reference (``heterogeneous_network.py:27-39``); ``**kwargs`` swallows
        ``ignored_label`` etc. exactly like the reference does."""
        super().__init__()
        assert conv_block in ["GraphSAGE", "GAT", "GAT_edge"]
        self.conv_block = conv_block
        if output_dim is not None:
            assert output_dim_dict is None
            self.classification_task = "room"
            output_dim_dict = {"rooms": output_dim, "objects": output_dim}  # final objects states are ignored
        else:
            assert output_dim_dict is not None
            self.classification_task = "all"  # two outputs: the executor's second readout (hmp_net_aux_output / hmp_net_backward2)
        self.num_layers = num_layers if conv_block[:3] != "GAT" else len(GAT_heads)
        self.dropout = dropout
        self.input_dim_dict = dict(input_dim_dict)

        hidden_dim_dict = {"rooms": hidden_dim, "objects": hidden_dim}
        if conv_block == "GAT":
            self.convs = build_GAT_hetero_conv(EDGE_TYPES, input_dim_dict, output_dim_dict, GAT_hidden_dims, GAT_heads,
                                               GAT_concats, dropout)
        elif conv_block == "GAT_edge":
            self.convs = build_GAT_hetero_conv(EDGE_TYPES, input_dim_dict, output_dim_dict, GAT_hidden_dims, GAT_heads,
                                               GAT_concats, dropout, edge_dim=3,
                                               fill_value=torch.zeros(3, dtype=torch.float64))
        else:
            dims = [input_dim_dict] + [hidden_dim_dict] * (self.num_layers - 1) + [output_dim_dict]
            self.convs = nn.ModuleList(
                build_hetero_conv(conv_block, EDGE_TYPES, dims[l], dims[l + 1]) for l in range(self.num_layers))
        self._init_native()

    def _build_native(self) -> NativeNet:
        node_types = ["objects", "rooms"]
        two = self.classification_task == "all"
        tail = ((ACT_ELU if self.conv_block[:3] == "GAT" else ACT_RELU), float(self.dropout)) if two else None
        return NativeNet(node_types, self.input_dim_dict, EDGE_TYPES, _hetero_layers(self, node_types), readout="rooms",
                         aux_readout="objects" if two else None, tail=tail)

    _EXPLAIN_EDGE = ("objects", "objects_to_rooms", "rooms")

    def explain_rooms(self, data, k=3, by="attention", target=None, wrt="logit"):
        """Which objects a room's label rests on, on the host: ``(objects int64 [rooms, k], weight float32 [rooms, k])``, ``-1`` /
        ``0`` past a room's objects (views of one pinned buffer: valid until the next call), moved by one device-to-host copy.

        ``by="attention"`` (the default; GAT / GAT_edge models only, which keep returning what they returned): for every room
        the ``k`` most attended objects of the last layer's ``objects_to_rooms`` conv and their weights (:meth:`top_attended`).
        ``by="gradient"`` (GraphSAGE, GAT and GAT_edge models): the ``k`` objects with the largest ``|gradient x input|`` of the
        room's own predicted-class logit (``target`` / ``wrt`` as :meth:`input_gradients` takes them) with the signed score --
        exact per-room passes, one per room ordinal of the batch's graphs (a single frame is one graph), all queued without a
        host synchronisation into one output."""
        if by not in ("attention", "gradient"):
            raise _lib.HydraMPError(f"explain_rooms: by must be 'attention' or 'gradient', got {by!r}")
        if by == "gradient":
            return self._explain_by_gradient(data, k, target=target, wrt=wrt)
        if self.conv_block[:3] != "GAT":
            raise _lib.HydraMPError(f"explain_rooms: no attention coefficients: conv_block {self.conv_block} has no attention (GAT and "
                                    "GAT_edge models export them); explain_rooms(by='gradient') ranks the objects by gradient x "
                                    "input on every model")
        l = self._attention_layer(-1, "explain_rooms")
        _lib.require_device()  # no device: HydraMPError (there is no CPU fallback)
        return self.native().explain(data, l, self._EXPLAIN_EDGE, k)

    def forward(self, data):
        out = self._run(data)
        dims = self.native().layers[-1].out_dims
        if self.classification_task == "room":
            return out[:, : dims["rooms"]]
        rooms, objects = out
        last = self.num_layers - 1
        return (self._tail_act_drop(rooms[:, : dims["rooms"]], self._drop_stream(last, "rooms")),
                self._tail_act_drop(objects[:, : dims["objects"]], self._drop_stream(last, "objects")))
