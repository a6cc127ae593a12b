"""Device-resident dataset + device-side collation.

The reference feeds the training loop through PyG's ``DataLoader`` (``base_training_job.py:164-178``): every step it
collates ``batch_size`` ``HeteroData`` objects on the host (``Batch.from_data_list``) and copies the result to the device
(``batch.to(device)``, :205).  With the native step at ~0.1 ms that host work dominates.  :class:`GraphStore` uploads the
whole list of graphs ONCE as packed per-type arrays (MP3D: 90 scenes x 5 trajectories of 10^2-node graphs -- a few hundred
MB) and :meth:`GraphStore.collate` assembles a batch with the gather kernels of ``csrc/collate.hip``
(``hmp_collate_rows`` / ``hmp_collate_edges``).  The host only computes the ``[B + 1]`` offset vectors of the batch (numpy
cumsums over per-graph counts it keeps) and ships them in ONE small pinned H2D copy.

The result is a :class:`hydra_gnn_amd.data.HeteroData` on the device with the same content, order and dtypes as
``data.collate(graphs).to(device)`` (bit-identical: ``tests/test_gpu_collate.py``), incl. ``batch`` / ``ptr`` vectors and
``num_graphs``.

The two-headed (room + object) task of ``SemiSupervisedTrainingJob`` (``semisupervised_training_job.py:89-160``) is served the
same way: bool / int8 rows (``train_mask`` / ``val_mask`` / ``test_mask`` / ``room_mask`` / ``object_mask``) are stored as they
are and move through the byte branch of the same kernels, and a list of homogeneous :class:`hydra_gnn_amd.data.Data` graphs is
stored under the names the homogeneous models present to the executor (node type ``node``; ``edge_index`` -> ``to``,
``pool_edge_index`` -> ``pool``, ``init_edge_index`` -> ``init``).  A stream created for a two-headed model carries the labels and
masks of both heads in its own buffers (``tests/test_gpu_semisupervised_stream.py``); a stream created for a homogeneous room
classifier carries ``room_mask`` and the room-masked labels (``tests/test_gpu_homog_room_stream.py``).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .data import Data, EdgeType, HeteroData

# homogeneous graphs: the names of the models' views (models/homogeneous_network.py, homogeneous_neural_tree_network.py)
HOMO_NODE = "node"
_HOMO_REL = {"edge_index": "to", "pool_edge_index": "pool", "init_edge_index": "init"}
_HOMO_EDGE_ROWS = ("edge_attr", "edge_type")  # per-edge rows that follow `edge_index`
DEFAULT_MASKS = ("train_mask", "val_mask", "test_mask")


def homo_edge_type(name: str) -> EdgeType:
    """edge type under which a homogeneous ``*index*`` attribute is stored"""
    rel = _HOMO_REL.get(name) or name.replace("_edge_index", "").replace("_index", "")
    return (HOMO_NODE, rel, HOMO_NODE)


class _Packed:
    """all graphs' rows of one attribute back to back + [G + 1] row offsets (host copy kept for the offset arithmetic)"""

    def __init__(self, parts: List[torch.Tensor], device):
        self.counts = np.array([int(p.size(0)) for p in parts], dtype=np.int64)
        self.ptr_host = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        self.data = torch.cat(parts, dim=0).contiguous().to(device)
        self.ptr = torch.from_numpy(self.ptr_host).to(device)
        self.row_shape = tuple(self.data.shape[1:])
        # any size: multiples of 4 move as 4-byte units, bool / int8 rows byte by byte (csrc/collate.hip)
        self.row_bytes = int(self.data.element_size()) * (int(np.prod(self.row_shape, dtype=np.int64)) if self.row_shape else 1)


def _packed(data: torch.Tensor, ptr: torch.Tensor, ptr_host: np.ndarray) -> _Packed:
    """a ``_Packed`` over rows that are already back to back on the device, with their ``[G + 1]`` offsets (device and host)"""
    pk = object.__new__(_Packed)
    ptr_host = np.ascontiguousarray(ptr_host, dtype=np.int64)
    pk.counts, pk.ptr_host = np.diff(ptr_host), ptr_host
    pk.data, pk.ptr = data, ptr
    pk.row_shape = tuple(data.shape[1:])
    pk.row_bytes = int(data.element_size()) * (int(np.prod(pk.row_shape, dtype=np.int64)) if pk.row_shape else 1)
    return pk


class GraphStore:
    def __init__(self, graphs: Sequence, device="cuda:0"):
        """``graphs``: a list of ``HeteroData``, or a list of homogeneous ``Data`` (classified by name as PyG and
        ``data.collate_homogeneous`` do: ``*index*`` = an edge list shifted by the node offsets, ``edge_attr`` / ``edge_type`` = rows
        per edge of ``edge_index``, every other tensor = rows per node)."""
        assert len(graphs) > 0
        self.device = torch.device(device)
        self.lib = _lib.require_device()
        self.n_graphs = len(graphs)
        g0 = graphs[0]
        self.homogeneous = not hasattr(g0, "node_types")
        self._stage = None
        self._stage_dev = None
        self._copied = None  # event: the previous batch's offset copy has left the pinned buffer
        self.edge_rows: Dict[EdgeType, Dict[str, _Packed]] = {}  # per-edge rows by attribute name (edge_attr, edge_type)
        if self.homogeneous:
            self._init_homogeneous(graphs)
            return
        self.node_types = list(g0.node_types)
        self.edge_types: List[EdgeType] = list(g0.edge_types)
        # node attributes (tensors whose first dimension is the node count)
        self.node_attrs: Dict[str, Dict[str, _Packed]] = {}
        self.node_counts: Dict[str, np.ndarray] = {}
        self.count_only: Dict[str, bool] = {}
        for t in self.node_types:
            keys = [k for k in g0[t].keys() if isinstance(getattr(g0[t], k), torch.Tensor)]
            self.node_attrs[t] = {}
            for k in keys:
                self.node_attrs[t][k] = _Packed([getattr(g[t], k) for g in graphs], self.device)
            self.node_counts[t] = np.array([int(g[t].num_nodes) for g in graphs], dtype=np.int64)
            self.count_only[t] = "num_nodes" in g0[t] and "x" not in g0[t]
        # edges: graph-local indices, [2][E_total]
        self.edge_index: Dict[EdgeType, torch.Tensor] = {}
        self.edge_ptr: Dict[EdgeType, torch.Tensor] = {}
        self.edge_ptr_host: Dict[EdgeType, np.ndarray] = {}
        self.edge_attr: Dict[EdgeType, _Packed] = {}
        for e in self.edge_types:
            eis = [g[e].edge_index.to(torch.int64) for g in graphs]
            counts = np.array([int(ei.size(1)) for ei in eis], dtype=np.int64)
            ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
            self.edge_ptr_host[e] = ptr
            self.edge_ptr[e] = torch.from_numpy(ptr).to(self.device)
            self.edge_index[e] = torch.cat(eis, dim=1).contiguous().to(self.device)
            if "edge_attr" in g0[e]:
                self.edge_attr[e] = _Packed([g[e].edge_attr for g in graphs], self.device)
                self.edge_rows[e] = {"edge_attr": self.edge_attr[e]}

    def _init_homogeneous(self, graphs: Sequence[Data]) -> None:
        g0 = graphs[0]
        keys = [k for k, v in g0.__dict__.items() if k != "_plan_cache" and isinstance(v, torch.Tensor)]
        self.homo_keys = keys  # collate_homogeneous's attribute order
        if "x" not in keys:
            raise _lib.HydraMPError("homogeneous graphs need the node features 'x' (they give the node count)")
        self.node_types = [HOMO_NODE]
        self.node_counts = {HOMO_NODE: np.array([int(g.num_nodes) for g in graphs], dtype=np.int64)}
        self.count_only = {HOMO_NODE: False}
        self.node_attrs = {HOMO_NODE: {}}
        self.edge_types, self.edge_name = [], {}
        self.edge_index, self.edge_ptr, self.edge_ptr_host, self.edge_attr = {}, {}, {}, {}
        for k in keys:
            parts = [getattr(g, k) for g in graphs]
            if "index" in k:
                e = homo_edge_type(k)
                if e in self.edge_name:
                    raise _lib.HydraMPError(f"attributes '{self.edge_name[e]}' and '{k}' map to the same edge type {e}")
                counts = np.array([int(ei.size(1)) for ei in parts], dtype=np.int64)
                ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
                self.edge_types.append(e)
                self.edge_name[e] = k
                self.edge_ptr_host[e] = ptr
                self.edge_ptr[e] = torch.from_numpy(ptr).to(self.device)
                if parts[0].dtype != torch.int64:
                    raise _lib.HydraMPError(f"'{k}' must be int64, got {parts[0].dtype}")
                self.edge_index[e] = torch.cat(parts, dim=1).contiguous().to(self.device)
            elif k not in _HOMO_EDGE_ROWS:
                pk = _Packed(parts, self.device)
                if not np.array_equal(pk.counts, self.node_counts[HOMO_NODE]):
                    raise _lib.HydraMPError(f"'{k}' is stored per node but its first dimension is not the node count of every graph")
                self.node_attrs[HOMO_NODE][k] = pk
        for k in keys:
            if k in _HOMO_EDGE_ROWS:
                e = homo_edge_type("edge_index")
                if e not in self.edge_name:
                    raise _lib.HydraMPError(f"'{k}' without 'edge_index'")
                pk = _Packed([getattr(g, k) for g in graphs], self.device)
                if not np.array_equal(pk.counts, np.diff(self.edge_ptr_host[e])):
                    raise _lib.HydraMPError(f"'{k}' must have one row per edge of 'edge_index' in every graph")
                self.edge_rows.setdefault(e, {})[k] = pk
                if k == "edge_attr":
                    self.edge_attr[e] = pk

    @classmethod
    def from_frames(cls, pipeline, frames, y=None):
        """``(store, infos)``: a store over the frames that have a room and a kept object, straight from scene-graph arrays -- what
        ``GraphStore([clone of pipeline.convert(*f)[0] (+ y) for f in frames])`` holds, packed array for packed array and offset
        vector for offset vector, without the per-frame launches, clones and ``torch.cat``s: the frames go through the pipeline's
        batch path in store form (``HMP_FB_STORE``: rows back to back, graph-LOCAL edge lists, ``[G + 1]`` offsets; one host stage,
        one upload and one launch per chunk).  ``frames`` / ``y`` / ``infos`` as ``FramePipeline.convert_batch`` (``infos[i]["graph"]``
        is the frame's index in the store).  Frames beyond the capacity of one launch's tables are converted in chunks, and the
        chunks are joined with ``torch.cat`` here: once per dataset, at construction, not on a hot path.  The store owns COPIES:
        nothing it holds is a view of the pipeline's arena, so the pipeline stays free for other frames."""
        from . import dsg

        lib = pipeline._lib
        built, infos = pipeline._build_frames(frames)
        try:
            live = [i for i, info in enumerate(infos) if info is not None]
            if not live:
                raise _lib.HydraMPError("GraphStore.from_frames: no frame has a room and a kept object")
            cap = pipeline._batch_capacity(built[live[0]][0], _lib.FB_STORE, y is not None)
            if cap < 1:
                raise _lib.HydraMPError("GraphStore.from_frames: one frame does not fit the launch's tables")
            chunks = []
            for c in range(0, len(live), cap):
                idx = live[c:c + cap]
                sub_infos = [infos[i] for i in idx]
                tensors, host = pipeline._run_batch([built[i] for i in idx], None if y is None else [y[i] for i in idx], _lib.FB_STORE,
                                                    sub_infos)
                for info in sub_infos:
                    info["graph"] += c
                chunks.append(({t: v.clone() for t, v in tensors.items()}, host))  # the arena is rewritten by the next chunk
        finally:
            for h, _ in built:
                lib.hmp_frame_destroy(h)
        FB = _lib.FT_BATCH

        def joined_ptr(t, host_key, k):
            dev = torch.cat([ch[t] if i == 0 else ch[t][1:] + int(sum(c[1][host_key][k][-1] for c in chunks[:i]))
                             for i, (ch, _) in enumerate(chunks)])
            hst = np.concatenate([h[host_key][k] if i == 0 else h[host_key][k][1:] + sum(c[1][host_key][k][-1] for c in chunks[:i])
                                  for i, (_, h) in enumerate(chunks)]).astype(np.int64)
            return dev, hst

        data = {t: torch.cat([ch[t] for ch, _ in chunks], dim=1 if v.dim() == 2 and v.dtype == torch.int64 else 0) if len(chunks) > 1 else v
                for t, v in chunks[0][0].items() if not FB + _lib.FTB_NODE_PTR <= t < FB + _lib.FTB_Y}  # the offset vectors are joined below
        ht, homog = pipeline.htree, pipeline.homogeneous
        node_names, edge_names = dsg._node_type_names(ht, homog), dsg._edge_type_names(ht, homog)
        node_ptr = [joined_ptr(FB + _lib.FTB_NODE_PTR + k, "node_ptr", k) for k in range(len(node_names))]
        edge_ptr = [joined_ptr(FB + _lib.FTB_EDGE_PTR + k, "edge_ptr", k) for k in range(len(edge_names))]

        self = object.__new__(cls)
        self.device, self.lib = pipeline.device, _lib.require_device()
        self.n_graphs, self.homogeneous = len(live), homog
        self._stage = self._stage_dev = self._copied = None
        self.edge_rows, self.edge_index, self.edge_ptr, self.edge_ptr_host, self.edge_attr = {}, {}, {}, {}, {}
        self.count_only = {t: False for t in ([HOMO_NODE] if homog else node_names)}
        if homog:
            names = {t: ("y" if t == FB + _lib.FTB_Y else dsg._HOMOG_TENSORS[t - _lib.FT_HOMOG]) for t in data}
            self.homo_keys = [names[t] for t in sorted(data)]  # the attribute order of the pipeline's Data, then y
            self.node_types, self.node_counts = [HOMO_NODE], {HOMO_NODE: np.diff(node_ptr[0][1])}
            self.node_attrs, self.edge_types, self.edge_name = {HOMO_NODE: {}}, [], {}
            e0 = homo_edge_type("edge_index")
            for t in sorted(data):
                k = names[t]
                if "index" in k:
                    e = homo_edge_type(k)
                    self.edge_types.append(e)
                    self.edge_name[e] = k
                    self.edge_index[e] = data[t]
                    self.edge_ptr[e], self.edge_ptr_host[e] = edge_ptr[edge_names.index(k)]
                elif k not in _HOMO_EDGE_ROWS:
                    self.node_attrs[HOMO_NODE][k] = _packed(data[t], *node_ptr[0])
            for t in sorted(data):
                if names[t] in _HOMO_EDGE_ROWS:
                    pk = _packed(data[t], self.edge_ptr[e0], self.edge_ptr_host[e0])
                    self.edge_rows.setdefault(e0, {})[names[t]] = pk
                    if names[t] == "edge_attr":
                        self.edge_attr[e0] = pk
            return self, infos
        self.node_types, self.edge_types = list(node_names), list(edge_names)
        self.node_attrs = {t: {} for t in node_names}
        self.node_counts = {t: np.diff(node_ptr[k][1]) for k, t in enumerate(node_names)}
        for t in sorted(data):
            if FB <= t < _lib.FT_HTREL:
                k = t - FB - _lib.FTB_Y
                self.node_attrs[node_names[k]]["y"] = _packed(data[t], *node_ptr[k])
                continue
            key, attr = dsg._typed_tensor(t)  # sorted: an edge type's edge_index comes before its edge_attr
            if attr == "edge_index":
                self.edge_index[key] = data[t]
                self.edge_ptr[key], self.edge_ptr_host[key] = edge_ptr[edge_names.index(key)]
            elif attr == "edge_attr":
                self.edge_attr[key] = _packed(data[t], self.edge_ptr[key], self.edge_ptr_host[key])
                self.edge_rows[key] = {"edge_attr": self.edge_attr[key]}
            else:
                self.node_attrs[key][attr] = _packed(data[t], *node_ptr[node_names.index(key)])
        return self, infos

    # ---------------------------------------------------------------------------------------------------------------
    def collate(self, ids: Sequence[int]):
        """Batch of graphs ``ids`` (in that order) on the device; equals ``data.collate([graphs[i] for i in ids]).to(device)``
        (a store of homogeneous graphs: ``data.collate_homogeneous(...).to(device)``, a ``Data``)."""
        sel_host = np.asarray(ids, dtype=np.int64)
        B = int(sel_host.size)
        assert B > 0 and sel_host.min() >= 0 and sel_host.max() < self.n_graphs
        st = _lib.stream_ptr()
        # ---- host: offsets of every node / edge type in the batch, packed into one int64 staging vector
        node_off: Dict[str, np.ndarray] = {}
        for t in self.node_types:
            node_off[t] = np.concatenate([[0], np.cumsum(self.node_counts[t][sel_host])]).astype(np.int64)
        edge_off: Dict[EdgeType, np.ndarray] = {}
        for e in self.edge_types:
            p = self.edge_ptr_host[e]
            edge_off[e] = np.concatenate([[0], np.cumsum(p[sel_host + 1] - p[sel_host])]).astype(np.int64)
        n_vec = len(self.node_types) + len(self.edge_types)
        words = n_vec * (B + 1) + (B + 1) // 2 + 1  # + sel as int32
        if self._copied is not None:
            self._copied.synchronize()  # the pinned buffer is about to be rewritten
        if self._stage is None or self._stage.numel() < words:
            self._stage = torch.empty(max(words, 4096), dtype=torch.int64).pin_memory()
            self._stage_dev = torch.empty_like(self._stage, device=self.device)
            self._copied = torch.cuda.Event()
        stage = self._stage.numpy()
        pos, where = 0, {}
        for key, vec in list(node_off.items()) + list(edge_off.items()):
            stage[pos:pos + B + 1] = vec
            where[key] = pos
            pos += B + 1
        sel32 = stage[pos:pos + (B + 1) // 2 + 1].view(np.int32)
        sel32[:B] = sel_host.astype(np.int32)
        sel_pos = pos
        self._stage_dev[:words].copy_(self._stage[:words], non_blocking=True)
        self._copied.record()
        dev = self._stage_dev
        sel_ptr = dev[sel_pos:].data_ptr()
        off_ptr = lambda key: dev[where[key]:].data_ptr()

        out = HeteroData()
        out.num_graphs = B
        lib = self.lib
        for t in self.node_types:
            n_out = int(node_off[t][-1])
            for k, pk in self.node_attrs[t].items():
                dst = torch.empty((n_out,) + pk.row_shape, dtype=pk.data.dtype, device=self.device)
                _lib.check(lib.hmp_collate_rows(pk.data.data_ptr(), pk.row_bytes, pk.ptr.data_ptr(), sel_ptr, off_ptr(t), B, n_out,
                                                dst.data_ptr(), st))
                setattr(out[t], k, dst)
            if self.count_only[t]:
                out[t].num_nodes = n_out
            if self.homogeneous:  # collate_homogeneous keeps no batch / ptr vectors
                continue
            ptr = dev[where[t]:where[t] + B + 1].clone()
            out[t].ptr = ptr
            out[t].batch = torch.repeat_interleave(torch.arange(B, dtype=torch.int64, device=self.device), ptr[1:] - ptr[:-1],
                                                   output_size=n_out)
        for e in self.edge_types:
            e_out = int(edge_off[e][-1])
            dst = torch.empty((2, e_out), dtype=torch.int64, device=self.device)
            src = self.edge_index[e]
            _lib.check(lib.hmp_collate_edges(src.data_ptr(), int(src.size(1)), self.edge_ptr[e].data_ptr(), sel_ptr, off_ptr(e),
                                             off_ptr(e[0]), off_ptr(e[2]), B, e_out, dst.data_ptr(), st))
            out[e].edge_index = dst
            for k, pk in self.edge_rows.get(e, {}).items():
                ea = torch.empty((e_out,) + pk.row_shape, dtype=pk.data.dtype, device=self.device)
                _lib.check(lib.hmp_collate_rows(pk.data.data_ptr(), pk.row_bytes, self.edge_ptr[e].data_ptr(), sel_ptr, off_ptr(e), B, e_out,
                                                ea.data_ptr(), st))
                setattr(out[e], k, ea)
        if not self.homogeneous:
            return out
        flat = Data()
        e0 = homo_edge_type("edge_index")
        for k in self.homo_keys:
            if "index" in k:
                flat.__dict__[k] = out[homo_edge_type(k)].edge_index
            elif k in _HOMO_EDGE_ROWS:
                flat.__dict__[k] = getattr(out[e0], k)
            else:
                flat.__dict__[k] = getattr(out[HOMO_NODE], k)
        flat.num_graphs = B
        return flat


class BatchStream:
    """A DataLoader's inner loop for ONE network, without the DataLoader: every :meth:`next` assembles a fresh batch of
    ``batch_size`` graphs on the device (``hmp_collator_run``: one host call, one kernel, outputs in buffers allocated once) and
    hands back the executor's batch descriptor ready made -- no per-tensor Python between two training steps
    (``base_training_job.py:202-216`` spends it in ``DataLoader.__next__`` + ``batch.to(device)`` + ``make_batch``).

        stream = store.stream(model, batch_size=32, label_type="rooms")
        for ids in sampler:                  # e.g. a shuffled permutation cut into batches
            step.run(stream.next(ids))       # TrainStep.run: fwd + loss + bwd + Adam on that batch

    Two-headed task (a model built with ``output_dim_dict``; no ``label_type``): the stream collates, in the same launch, the
    features and edges the net reads plus ``y`` and the ``masks`` of both heads (homogeneous models: ``room_mask`` and, for
    H-trees, ``object_mask`` too), and nothing else the store holds:

        stream = store.stream(model, batch_size=64)
        step = model.semisupervised_step(lr, use_graph=False)
        for ids in sampler:
            step.run(stream.next(ids), mask="train_mask")
        acc = evaluate.semisupervised_accuracy(model, (stream, id_lists), "val_mask")

    Room task on a store of homogeneous graphs (a ``HomogeneousNetwork`` / ``HomogeneousNeuralTreeNetwork`` built with
    ``output_dim``; ``label_type="node"``): the stream collates ``x``, the edge lists (and ``edge_attr``) the net reads, ``room_mask``
    and ``y``, the latter as the labels the fused step reads -- ``room_mask ? y : ignored_label``, written by the same launch
    (``hmp_collator_set_label_filter``).  ``stream.members`` is the collated ``room_mask``: the row filter of the counts.  A step or
    a count with another ``ignored_label`` than the stream's is refused.

        stream = store.stream(model, batch_size=64, label_type="node", ignored_label=25)
        step = model.train_step(lr, ignored_label=25, use_graph=False)
        step.run(stream.next(ids)); model.count_correct_rooms(stream.next(ids), counts)

    The buffers are reused by the next call: a batch is valid until then (same-stream ordering makes that safe for everything
    already enqueued).  ``stream.data()`` presents the current batch as a ``HeteroData`` of views for code that wants one."""

    def __init__(self, store: "GraphStore", net, batch_size: int, label_type: Optional[str] = None, label_key: str = "y",
                 masks: Sequence[str] = DEFAULT_MASKS, targets: bool = True, ignored_label: int = 25):
        import ctypes as C

        self.store, self.B = store, int(batch_size)
        self.net = net
        lib = store.lib
        dev = store.device
        nat = net.native() if hasattr(net, "native") else net
        self.nat = nat
        # two-headed task: the stream carries what the net reads plus the targets of both heads (labels, the named masks, the
        # head rows of the homogeneous models) and nothing else the store holds; room task: every attribute, as before
        self.two_headed = nat.aux_readout is not None or nat.heads is not None
        if self.two_headed and label_type is not None:
            raise _lib.HydraMPError("a two-headed model's stream carries the targets of both heads: pass no label_type")
        if not self.two_headed and label_type is None:
            raise _lib.HydraMPError("label_type is required: the node type whose labels the model's single output is trained on")
        # room task on homogeneous graphs: the net has an output row per node, so the stream carries `room_mask` (the rows that count)
        # and the labels the fused step reads, room_mask ? y : ignored_label, written by the collation launch (the label filter)
        self.homog_room = not self.two_headed and store.homogeneous
        self.ignored_label = int(ignored_label) if self.homog_room else None
        self.members = None
        self.mask_names = tuple(masks) if (self.two_headed and targets) else ()
        self._target_kind = None
        target_attrs: Dict[str, List[str]] = {}
        if self.homog_room:
            if getattr(net, "op_path", False):
                raise _lib.HydraMPError(f"{net.conv_block} runs op by op: there is no fused step to stream batches to")
            attrs = store.node_attrs[HOMO_NODE]
            if "room_mask" not in attrs:
                raise _lib.HydraMPError("the store holds no attribute 'room_mask' (the rows of the room task on homogeneous graphs)")
            if attrs["room_mask"].data.dtype != torch.bool or attrs["room_mask"].row_shape != ():
                raise _lib.HydraMPError(f"'room_mask' must be a bool vector (one entry per node), the store holds "
                                        f"{attrs['room_mask'].row_shape} {attrs['room_mask'].data.dtype}")
            if label_key not in attrs:
                raise _lib.HydraMPError(f"the store holds no attribute '{label_key}' of node type '{HOMO_NODE}'")
            if attrs[label_key].data.dtype != torch.int64 or attrs[label_key].row_shape != ():
                raise _lib.HydraMPError(f"'{label_key}' must be an int64 vector (one label per node), the store holds "
                                        f"{attrs[label_key].row_shape} {attrs[label_key].data.dtype}")
            target_attrs[HOMO_NODE] = [label_key, "room_mask"]
        # selective: the stream carries what the net reads plus its targets; otherwise every attribute the store holds -- as long
        # as that fits the collator's table.  A typed H-tree store with relative positions holds 50 arrays (20 node attributes, 15
        # edge lists, 15 edge_attr): its single-headed stream carries what the net reads and the labels, like the other two.
        selective = self.two_headed or self.homog_room
        if not selective:
            n_all = sum(len(a) for a in store.node_attrs.values()) + len(store.edge_types) + sum(e in store.edge_attr for e in store.edge_types)
            if n_all > _lib.COLLATE_MAX_ITEMS or len(store.node_types) + len(store.edge_types) > _lib.COLLATE_MAX_SLOTS:
                selective = True
                target_attrs[label_type] = [label_key]
        if self.two_headed and targets:
            if nat.heads is not None:  # learned linear heads over the rows of one node set
                self._target_kind = "linear"
                self._object_attr = getattr(net, "_OBJECT_ATTR", None)
                rows = ["room_mask"] + ([self._object_attr] if self._object_attr is not None else [])
                self._label_types = (nat.pool_edge_type[2] if nat.pool_edge_type is not None else nat.readout,)
                target_attrs[self._label_types[0]] = [label_key] + list(self.mask_names) + rows
            else:
                self._target_kind = "heads"
                self._label_types = tuple(nat.head_label_types())
                for t in self._label_types:
                    target_attrs[t] = [label_key] + list(self.mask_names)
        self._label_key = label_key
        if selective:
            used_nodes = set(nat.node_types) | set(target_attrs)
            node_types = [t for t in store.node_types if t in used_nodes]
            edge_types = [e for e in store.edge_types if e in nat.edge_types]
        else:
            node_types, edge_types = list(store.node_types), list(store.edge_types)
        for t in list(nat.node_types) + list(target_attrs):
            if t not in node_types:
                raise _lib.HydraMPError(f"the store holds no node type '{t}'")
        for e in nat.edge_types:
            if e not in edge_types:
                raise _lib.HydraMPError(f"the store holds no edge type {e}")
        slots: List[object] = node_types + edge_types
        slot_of = {k: i for i, k in enumerate(slots)}
        host_ptrs = []
        for t in node_types:
            host_ptrs.append(np.concatenate([[0], np.cumsum(store.node_counts[t])]).astype(np.int64))
        for e in edge_types:
            host_ptrs.append(np.ascontiguousarray(store.edge_ptr_host[e], dtype=np.int64))
        self._host_ptrs = host_ptrs
        self._node_ptr_dev = {t: torch.from_numpy(host_ptrs[slot_of[t]]).to(dev) for t in node_types}
        # capacity of a batch per slot: B times the largest graph (ids may repeat)
        self.cap = [int(np.diff(p).max()) * self.B for p in host_ptrs]
        items, self._bufs, self._what = [], [], []

        def node_item(t, k):
            pk = store.node_attrs[t].get(k)
            if pk is None:
                raise _lib.HydraMPError(f"the store holds no attribute '{k}' of node type '{t}'")
            items.append(_lib.CollateItem(pk.data.data_ptr(), self._node_ptr_dev[t].data_ptr(), 0, pk.row_bytes, slot_of[t], 0, 0))
            self._bufs.append(torch.empty((max(self.cap[slot_of[t]], 1),) + pk.row_shape, dtype=pk.data.dtype, device=dev))
            self._what.append(("node", t, k))

        for t in node_types:
            if selective:
                keys = (["x"] if nat.in_dims.get(t, 0) > 0 and t in nat.node_types else []) + target_attrs.get(t, [])
            else:
                keys = list(store.node_attrs[t])
            for k in keys:
                node_item(t, k)
        for e in edge_types:
            src = store.edge_index[e]
            it = _lib.CollateItem(src.data_ptr(), store.edge_ptr[e].data_ptr(), int(src.size(1)), 0, slot_of[e], slot_of[e[0]], slot_of[e[2]])
            items.append(it)
            self._bufs.append(torch.empty(2 * max(self.cap[slot_of[e]], 1), dtype=torch.int64, device=dev))
            self._what.append(("edge", e, "edge_index"))
            if selective and not nat.edge_dims.get(e, 0):
                continue
            if selective and e not in store.edge_attr:
                raise _lib.HydraMPError(f"the store holds no 'edge_attr' of edge type {e} (read by the model's GAT_edge convs)")
            if e in store.edge_attr:
                pk = store.edge_attr[e]
                items.append(_lib.CollateItem(pk.data.data_ptr(), store.edge_ptr[e].data_ptr(), 0, pk.row_bytes, slot_of[e], 0, 0))
                self._bufs.append(torch.empty((max(self.cap[slot_of[e]], 1),) + pk.row_shape, dtype=pk.data.dtype, device=dev))
                self._what.append(("edge", e, "edge_attr"))
        n_items = len(items)
        if n_items > _lib.COLLATE_MAX_ITEMS or len(slots) > _lib.COLLATE_MAX_SLOTS:
            raise _lib.HydraMPError(f"the stream would collate {n_items} arrays of {len(slots)} node and edge types per batch, one launch's "
                                    f"table holds {_lib.COLLATE_MAX_ITEMS} of {_lib.COLLATE_MAX_SLOTS}: {[w[1:] for w in self._what]}")
        self._items = (_lib.CollateItem * n_items)(*items)
        self._slot_ptr = (C.c_void_p * len(slots))(*[p.ctypes.data for p in host_ptrs])
        h = C.c_void_p()
        self._h = None
        _lib.check(lib.hmp_collator_create(len(slots), self._slot_ptr, store.n_graphs, n_items, self._items, C.byref(h)))
        self._h = h
        if self.homog_room:  # the label item comes out as room_mask ? y : ignored_label
            _lib.check(lib.hmp_collator_set_label_filter(h, self._what.index(("node", HOMO_NODE, label_key)),
                                                         store.node_attrs[HOMO_NODE]["room_mask"].data.data_ptr(), self.ignored_label))
        self._dst = (C.c_void_p * n_items)(*[b.data_ptr() for b in self._bufs])
        self._caps = (C.c_int64 * n_items)(*[self.cap[it.slot] for it in items])
        self._totals = (C.c_int64 * len(slots))()
        # Batch.ptr of every slot, written by the collation kernel (the sliced plan build reads the node types' rows)
        self._off_stride = self.B + 1
        self._offsets = torch.zeros(len(slots) * self._off_stride, dtype=torch.int64, device=dev)
        self._slots, self._slot_of = slots, slot_of
        # ---- the executor's descriptor, filled once; per batch only the counts change
        from .engine import _BatchHolder

        hd = _BatchHolder()
        buf_of = {w: b for w, b in zip(self._what, self._bufs)}
        self._buf_of = buf_of
        self._node_slot, self._edge_slot = [], []
        for i, t in enumerate(nat.node_types):
            self._node_slot.append(slot_of[t])
            if nat.in_dims.get(t, 0) > 0:
                if ("node", t, "x") not in buf_of:
                    raise _lib.HydraMPError(f"the store holds no attribute 'x' of node type '{t}'")
                x = buf_of[("node", t, "x")]
                if x.dtype != torch.float32 or x.dim() != 2 or x.size(1) != nat.in_dims[t]:
                    raise _lib.HydraMPError(f"store features of '{t}' are {tuple(x.shape[1:])} {x.dtype}, model expects {nat.in_dims[t]} float32")
                hd.c.d_x[i] = x.data_ptr()
                hd.c.ldx[i] = x.size(1)
        for i, e in enumerate(nat.edge_types):
            self._edge_slot.append(slot_of[e])
            hd.c.d_edge_index[i] = buf_of[("edge", e, "edge_index")].data_ptr()
            if nat.edge_dims.get(e, 0):
                if ("edge", e, "edge_attr") not in buf_of:
                    raise _lib.HydraMPError(f"the store holds no 'edge_attr' of edge type {e} (read by the model's GAT_edge convs)")
                ea = buf_of[("edge", e, "edge_attr")]
                if ea.dtype != torch.float32 or ea.dim() != 2 or ea.size(1) != nat.edge_dims[e]:
                    raise _lib.HydraMPError(f"store 'edge_attr' of {e} is {tuple(ea.shape[1:])} {ea.dtype}, model expects {nat.edge_dims[e]} float32")
                hd.c.d_edge_attr[i] = ea.data_ptr()
        out_type = nat.pool_edge_type[2] if nat.pool_edge_type is not None else nat.readout
        if not self.two_headed:
            if ("node", label_type, label_key) not in buf_of:
                raise _lib.HydraMPError(f"the store holds no attribute '{label_key}' of node type '{label_type}'")
            lab = buf_of[("node", label_type, label_key)]
            if lab.dtype != torch.int64:
                raise _lib.HydraMPError("labels in the store must be int64")
            hd.c.d_labels = lab.data_ptr()
            if out_type != label_type:
                raise _lib.HydraMPError(f"labels of '{label_type}' for a model that reads out '{out_type}'")
            self.label_buf = lab
            if self.homog_room:  # the row filter of the counts: the collated room_mask (H-tree model included, reference :96-109)
                self.members = buf_of[("node", HOMO_NODE, "room_mask")]
        else:
            for t, keys in target_attrs.items():
                for k in keys:
                    v = buf_of[("node", t, k)]
                    want = torch.int64 if k == label_key else torch.bool
                    if v.dtype != want or v.dim() != 1:
                        raise _lib.HydraMPError(f"'{k}' of node type '{t}' must be a {str(want).replace('torch.', '')} vector (one entry per "
                                                f"node), the store holds {tuple(v.shape[1:])} {v.dtype}")
        hd.keep = list(self._bufs) + [self._offsets]
        for i, t in enumerate(nat.node_types):
            hd.c.d_node_ptr[i] = self._offsets.data_ptr() + 8 * slot_of[t] * self._off_stride
        for i, e in enumerate(nat.edge_types):  # the collator's edge offsets: edges arrive graph by graph
            hd.c.d_edge_ptr[i] = self._offsets.data_ptr() + 8 * slot_of[e] * self._off_stride
        hd.c.max_graph_nodes = int(max(int(np.diff(host_ptrs[slot_of[t]]).max()) for t in node_types))
        hd.n_nodes = [0] * len(nat.node_types)
        hd.n_edges = [0] * len(nat.edge_types)
        self._out_slot = slot_of[out_type]
        hd.stream = self  # TwoHeadTrainStep.run / count_correct find the targets through the descriptor
        self.holder = hd
        self._targets: Dict[Optional[str], Tuple[object, object]] = {}
        # workspace sized once for the largest batch this stream can produce
        cap_h = _BatchHolder()
        cap_h.n_nodes = [self.cap[s] for s in self._node_slot]
        cap_h.n_edges = [self.cap[s] for s in self._edge_slot]
        flat = nat.flat_params()
        with torch.cuda.device(flat.device):
            nat._ensure_workspace(cap_h, flat.device)

    def targets(self, mask: Optional[str]):
        """``byref`` of the stream's ``hmp_head_targets`` / ``hmp_linear_head_targets`` under the mask called ``mask`` (None = every
        row).  The buffers never move, so each is built once per mask name."""
        import ctypes as C

        hit = self._targets.get(mask)
        if hit is not None:
            return hit[1]
        if self._target_kind is None:
            raise _lib.HydraMPError("the stream carries no targets" + (" (it was created with targets=False)" if self.two_headed else
                                                                        ": it feeds a single-output model (TrainStep.run)"))
        if mask is not None and mask not in self.mask_names:
            raise _lib.HydraMPError(f"the stream carries no mask '{mask}' (it was created with masks={self.mask_names})")
        buf = lambda t, k: self._buf_of[("node", t, k)].data_ptr()
        if self._target_kind == "heads":
            tg = _lib.HeadTargets()
            for i, t in enumerate(self._label_types):
                tg.d_labels[i] = buf(t, self._label_key)
                if mask is not None:
                    tg.d_mask[i] = buf(t, mask)
        else:
            t = self._label_types[0]
            tg = _lib.LinearHeadTargets()
            tg.d_labels = buf(t, self._label_key)
            if mask is not None:
                tg.d_mask = buf(t, mask)
            tg.d_member[0] = buf(t, "room_mask")
            if self._object_attr is not None:  # None: the object head's rows are the complement of the room rows
                tg.d_member[1] = buf(t, self._object_attr)
        self._targets[mask] = (tg, C.byref(tg))
        return self._targets[mask][1]

    def member_rows(self):
        """addresses of the collated head rows of a linear-head stream, (room rows, object rows or None = their complement): what
        :meth:`targets` holds, for the entries that take no labels (``NativeNet.predict_labels``)"""
        self.targets(None)
        tg = self._targets[None][0]
        if self._target_kind != "linear":
            raise _lib.HydraMPError("member_rows: the stream's heads are whole node types (no member rows)")
        return tg.d_member[0], tg.d_member[1]

    def next(self, ids) -> "object":
        """collate graphs ``ids`` (len == batch_size or fewer) into the stream's buffers; returns the descriptor for TrainStep.run"""
        sel = np.ascontiguousarray(ids, dtype=np.int32)
        B = int(sel.size)
        if B > self.B:
            raise _lib.HydraMPError(f"{B} graphs for a stream of batch size {self.B}")
        _lib.check(self.store.lib.hmp_collator_run(self._h, sel.ctypes.data, B, self._dst, self._caps, self._totals,
                                                   self._offsets.data_ptr(), self._off_stride, _lib.stream_ptr()))
        hd, tot = self.holder, self._totals
        for i, s in enumerate(self._node_slot):
            v = tot[s]
            hd.c.n_nodes[i] = v
            hd.n_nodes[i] = v
        for i, s in enumerate(self._edge_slot):
            v = tot[s]
            hd.c.n_edges[i] = v
            hd.n_edges[i] = v
        hd.c.n_out = tot[self._out_slot]
        hd.c.n_graphs = B
        self.num_graphs = B
        return hd

    def data(self) -> HeteroData:
        """the current batch as a HeteroData of VIEWS into the stream's buffers (valid until the next :meth:`next`)"""
        out = HeteroData()
        out.num_graphs = self.num_graphs
        for (kind, key, name), buf in zip(self._what, self._bufs):
            n = int(self._totals[self._slot_of[key]])
            if name == "edge_index":
                out[key].edge_index = buf[: 2 * n].view(2, n)
            else:
                setattr(out[key], name, buf[:n])
        return out

    def close(self):
        if getattr(self, "_h", None) is not None:
            self.store.lib.hmp_collator_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _graphstore_stream(self, net, batch_size: int, label_type: Optional[str] = None, label_key: str = "y",
                       masks: Sequence[str] = DEFAULT_MASKS, targets: bool = True, ignored_label: int = 25) -> BatchStream:
    return BatchStream(self, net, batch_size, label_type, label_key, masks, targets, ignored_label)


GraphStore.stream = _graphstore_stream
