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

A resident store is also where the configurations come from: ``with_relative_pos`` / ``to_homogeneous`` / ``remove_last_features`` /
``without_edge_types`` / ``zero_clique_features`` return the store of the transformed graphs from one launch of
``csrc/store_derive.hip``, ``generate_node_split`` writes the Stanford protocol's per-run masks in place, and :class:`StoreDataset` hands a store to the training jobs (second half of this module).
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
        FB, table = _lib.FT_BATCH, pipeline._tensors

        def joined_ptr(t, host_key, k):
            dev = torch.cat([ch[t] if i == 0 else ch[t][1:] + int(sum(c[1][host_key][k][-1] for c in chunks[:i]))
                             for i, (ch, _) in enumerate(chunks)])
            hst = np.concatenate([h[host_key][k] if i == 0 else h[host_key][k][1:] + sum(c[1][host_key][k][-1] for c in chunks[:i])
                                  for i, (_, h) in enumerate(chunks)]).astype(np.int64)
            return dev, hst

        data = {t: torch.cat([ch[t] for ch, _ in chunks], dim=1 if table[t][2] == dsg._EDGE else 0) if len(chunks) > 1 else v
                for t, v in chunks[0][0].items() if table[t][1] != "ptr"}  # the offset vectors are joined below
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
            names = {t: table[t][1] for t in data}
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
            key, attr, _ = table[t]  # sorted: an edge type's edge_index comes before its edge_attr
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

    def room_rows(self) -> torch.Tensor:
        """the collated ``room_mask`` buffer of a linear-head stream itself (capacity rows; the batch's rows lead), whose address
        :meth:`member_rows` returns first"""
        self.member_rows()
        return self._buf_of[("node", self._label_types[0], "room_mask")]

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
        hd.max_rows = {i: int(self.store.node_counts[t][sel].max()) for i, t in enumerate(self.nat.node_types)
                       if t in self.store.node_counts}
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


# =====================================================================================================================
# Label statistics of a resident store: the class histogram of the labels a training run reads and the class weights of the
# weighted cross entropy (``TrainStep.set_class_weight``), computed where the labels live -- two launches, no host read.
# =====================================================================================================================
CLASS_WEIGHT_SCHEMES = ("balanced",)
_NO_IGNORED = -(1 << 63)  # ignored_label=None: no label is ignored (the kernel compares with a value no class index takes)


def check_weight_scheme(scheme) -> str:
    if scheme not in CLASS_WEIGHT_SCHEMES:
        raise _lib.HydraMPError(f"class_weights: unknown scheme {scheme!r} (known: {', '.join(CLASS_WEIGHT_SCHEMES)})")
    return scheme


def balanced_weights_host(counts) -> np.ndarray:
    """Host statement of ``hmp_balanced_class_weights`` (scikit-learn's ``class_weight="balanced"`` over the classes present):
    ``w_c = N / (K * n_c)`` in float64 with ``N = sum n_c`` and ``K = #{c: n_c > 0}``, cast to float32; 0 for an absent class."""
    n = np.asarray(counts, dtype=np.int64)
    w = np.zeros(n.shape, dtype=np.float64)
    present = n > 0
    if present.any():
        w[present] = float(n.sum()) / (float(present.sum()) * n[present].astype(np.float64))
    return w.astype(np.float32)


def _label_rows(self: "GraphStore", who: str, label_type, label_key: str, mask):
    """(labels, row filter or None) of the rows a head trains on.  Typed stores: the rows of node type ``label_type``.  Homogeneous
    stores: ``label_type`` "rooms" (the default) = the rows of ``room_mask``, "objects" = the rows of ``object_mask`` (H-tree
    graphs) or the complement of ``room_mask`` -- the label filter of the stream and the member rows of the linear heads.
    ``mask`` names a bool attribute of those rows (``"train_mask"``: the node-split protocol) that narrows them further."""
    if self.homogeneous:
        attrs = self.node_attrs[HOMO_NODE]
        head = "rooms" if label_type is None else label_type
        if head not in ("rooms", "objects"):
            raise _lib.HydraMPError(f"{who}: label_type of a homogeneous store is 'rooms' or 'objects', got {label_type!r}")
        if "room_mask" not in attrs:
            raise _lib.HydraMPError(f"{who}: the store holds no attribute 'room_mask'")
        if head == "rooms":
            rows = attrs["room_mask"].data
        else:
            rows = attrs["object_mask"].data if "object_mask" in attrs else ~attrs["room_mask"].data
    else:
        if label_type is None:
            raise _lib.HydraMPError(f"{who}: label_type (the node type that carries the labels) is required for a typed store")
        if label_type not in self.node_attrs:
            raise _lib.HydraMPError(f"{who}: the store has no node type {label_type!r}")
        attrs, rows = self.node_attrs[label_type], None
    if label_key not in attrs:
        raise _lib.HydraMPError(f"{who}: the store holds no attribute {label_key!r} of those rows")
    lab = attrs[label_key].data
    if lab.dtype != torch.int64 or lab.dim() != 1:
        raise _lib.HydraMPError(f"{who}: {label_key!r} must be an int64 vector (one label per row), the store holds {tuple(lab.shape)} {lab.dtype}")
    if mask is not None:
        if mask not in attrs:
            raise _lib.HydraMPError(f"{who}: the store holds no mask {mask!r} of those rows (generate_node_split writes train_mask / val_mask / test_mask)")
        m = attrs[mask].data
        if m.dtype != torch.bool or m.shape != lab.shape:
            raise _lib.HydraMPError(f"{who}: {mask!r} must be a bool vector with one entry per row")
        rows = m if rows is None else (rows & m)
    if rows is not None and (rows.dtype != torch.bool or rows.shape != lab.shape):
        raise _lib.HydraMPError(f"{who}: the row filter must be a bool vector with one entry per row")
    return lab, (rows.contiguous() if rows is not None else None)


def _label_histogram(self: "GraphStore", who: str, label_type, label_key: str, mask, n_classes, ignored_label) -> torch.Tensor:
    if n_classes is None or int(n_classes) < 1:
        raise _lib.HydraMPError(f"{who}: n_classes (>= 1) is required")
    n_classes = int(n_classes)
    lab, rows = _label_rows(self, who, label_type, label_key, mask)
    counts = torch.zeros(n_classes + 1, dtype=torch.int64, device=self.device)
    ignored = _NO_IGNORED if ignored_label is None else int(ignored_label)
    with torch.cuda.device(self.device):
        _lib.check(self.lib.hmp_label_counts(lab.data_ptr(), lab.numel(), rows.data_ptr() if rows is not None else None, ignored,
                                             n_classes, counts.data_ptr(), _lib.stream_ptr()))
    return counts


def _class_counts(self: "GraphStore", label_type: Optional[str] = None, label_key: str = "y", mask: Optional[str] = None,
                  n_classes: Optional[int] = None, ignored_label: Optional[int] = None) -> torch.Tensor:
    """Class histogram of the store's labels (``hmp_label_counts``, one launch, nothing synchronises): device int64 ``[n_classes]``,
    entry ``c`` = the rows of label ``c`` among the rows :func:`_label_rows` describes whose label is not ``ignored_label``.  The
    result's attribute ``out_of_range`` (a device int64 scalar) counts the labels outside ``[0, n_classes)``."""
    counts = _label_histogram(self, "class_counts", label_type, label_key, mask, n_classes, ignored_label)
    out = counts[:-1]
    out.out_of_range = counts[-1]
    return out


def _class_weights(self: "GraphStore", label_type: Optional[str] = None, label_key: str = "y", mask: Optional[str] = None,
                   n_classes: Optional[int] = None, ignored_label: Optional[int] = None, scheme: str = "balanced") -> torch.Tensor:
    """Class weights from :meth:`class_counts`, device float32 ``[n_classes]``, ready for ``train_step(class_weight=...)``.
    ``scheme="balanced"``: ``w_c = N / (K * n_c)`` over the K classes present (N their rows; scikit-learn's "balanced"), 0 for an
    absent class (``hmp_balanced_class_weights``).  Two launches, no host read between them."""
    check_weight_scheme(scheme)
    counts = _label_histogram(self, "class_weights", label_type, label_key, mask, n_classes, ignored_label)
    w = torch.empty(int(n_classes), dtype=torch.float32, device=self.device)
    with torch.cuda.device(self.device):
        _lib.check(self.lib.hmp_balanced_class_weights(counts.data_ptr(), int(n_classes), w.data_ptr(), _lib.stream_ptr()))
    return w


GraphStore.class_counts = _class_counts
GraphStore.class_weights = _class_weights


# =====================================================================================================================
# Derived stores: the reference derives every configuration from ONE loaded dataset in place (train_mp3d.py:130-137,
# train_Stanford.py:87-99: compute_relative_pos for GAT_edge, to_homogeneous, remove_last_features for --remove_word2vec) and
# draws a node split per run (train_Stanford.py:166-171).  A resident store does the same without host graphs: the host
# plans destination offsets and an item table in numpy over the offset vectors the store keeps, uploads both in one block,
# and ``hmp_store_derive`` (csrc/store_derive.hip) writes every output in ONE launch.
# =====================================================================================================================
def _derive_alloc(shape, dtype, device) -> torch.Tensor:
    """every output of a derive launch and every mask row of a node split is allocated here (the tests patch it to pre-fill the
    outputs, so that an element the launch never writes cannot pass by luck)"""
    return torch.empty(shape, dtype=dtype, device=device)


def plan_concat(counts: Sequence[np.ndarray]):
    """Per-graph concatenation of ``len(counts)`` parts (node types of a homogeneous graph, edge types of one edge list), part
    after part inside a graph and graph after graph: ``counts[p][g]`` rows of part ``p`` in graph ``g``.  Returns
    ``(ptr [G + 1], inside [P][G], dst [P][G])``: the row offsets of the graphs in the concatenation, where part ``p`` starts inside
    graph ``g``'s range, and the same as an absolute row -- what ``torch.cat`` of every graph's parts, then of the graphs, lays out
    (``data.heterogeneous_data_to_homogeneous`` followed by ``GraphStore``).  Pure numpy; no part: ``ptr`` needs ``n_graphs``."""
    c = np.asarray(counts, dtype=np.int64)
    assert c.ndim == 2 and c.shape[0] > 0
    inside = np.cumsum(c, axis=0) - c
    ptr = np.concatenate([[0], np.cumsum(c.sum(axis=0))]).astype(np.int64)
    return ptr, inside, inside + ptr[:-1][None, :]


def _unit_of(*byte_values: int) -> int:
    """the widest unit (16 / 4 / 1 bytes) that divides every width, skip and base address of a rows item"""
    for u in (16, 4):
        if all(int(v) % u == 0 for v in byte_values):
            return u
    return 1


class DerivePlan:
    """The item table and the offset vectors of one ``hmp_store_derive`` launch, planned without a device: arrays enter by address
    (plain ints), offset vectors as numpy arrays that :meth:`pack` lays out behind the item table.  An item is a list of
    ``_lib.SD_ITEM_WORDS`` ints whose vector fields hold ``("vec", index)`` until :meth:`pack` resolves them."""

    THREADS, MAX_BLOCKS = 256, 1024

    def __init__(self, n_graphs: int):
        self.G = int(n_graphs)
        self.items: List[list] = []
        self.work: List[int] = []  # threads' worth of work per item (destination units / rows / edges)
        self.vectors: List[np.ndarray] = []
        self._seen: Dict[bytes, int] = {}

    def vector(self, v) -> Tuple[str, int]:
        v = np.ascontiguousarray(v, dtype=np.int64)
        key = v.tobytes()
        if key not in self._seen:
            self._seen[key] = len(self.vectors)
            self.vectors.append(v)
        return ("vec", self._seen[key])

    def _item(self, kind, work, **f):
        it = [0] * _lib.SD_ITEM_WORDS
        it[_lib.SD_KIND] = kind
        for k, v in f.items():
            it[getattr(_lib, "SD_" + k)] = v
        self.items.append(it)
        self.work.append(int(work))

    def rows(self, src: int, dst: int, src_ptr: int, dst_off, n: int, src_bytes: int, skip_bytes: int, take_bytes: int, dst_bytes: int):
        """rows of ``src_bytes`` bytes -> rows of ``dst_bytes``: bytes ``[skip, skip + take)`` then zeros; ``dst_off`` [G] = where a
        graph's rows start in the destination"""
        assert 0 <= skip_bytes and 0 <= take_bytes <= dst_bytes and skip_bytes + take_bytes <= src_bytes
        if n == 0 or dst_bytes == 0:
            return
        u = _unit_of(src_bytes, skip_bytes, take_bytes, dst_bytes, src, dst)
        self._item(_lib.SD_ROWS, n * (dst_bytes // u), SRC=src, DST=dst, SRC_PTR=src_ptr, DST_OFF=self.vector(dst_off), N=n,
                   SRC_W=src_bytes // u, SKIP=skip_bytes // u, TAKE=take_bytes // u, DST_W=dst_bytes // u, UNIT=u)

    def fill(self, dst: int, count_ptr: int, dst_off, n: int, value: int, unit: int):
        assert unit in (1, 8)
        if n:
            self._item(_lib.SD_FILL, n, DST=dst, SRC_PTR=count_ptr, DST_OFF=self.vector(dst_off), N=n, A0=int(value), UNIT=unit)

    def edges(self, src: int, dst: int, edge_ptr: int, dst_off, n: int, shift_src, shift_dst, dst_total: int):
        if n:
            self._item(_lib.SD_EDGES, n, SRC=src, DST=dst, SRC_PTR=edge_ptr, DST_OFF=self.vector(dst_off), N=n, A0=self.vector(shift_src),
                       A1=self.vector(shift_dst), A3=int(dst_total), UNIT=8)

    def relpos(self, edge_index: int, dst: int, edge_ptr: int, n: int, pos_src: int, pos_dst: int, ptr_src: int, ptr_dst: int):
        if n:
            self._item(_lib.SD_RELPOS, n, SRC=edge_index, DST=dst, SRC_PTR=edge_ptr, N=n, A0=pos_src, A1=pos_dst, A2=ptr_src, A3=ptr_dst,
                       UNIT=4)

    def compact(self, src: int, dst: int, src_ptr: int, dst_off, n: int, row_bytes: int, key: int, key_set: int):
        """the rows of ``row_bytes`` bytes whose int64 ``key`` (one per source row) is not in the 64-bit ``key_set``, graph by graph in
        source order from row ``dst_off[g]`` on: a wave per graph"""
        assert 0 <= key_set < 1 << 64 and row_bytes > 0
        if n == 0:
            return
        u = 8 if row_bytes % 8 == 0 and src % 8 == 0 and dst % 8 == 0 else 4
        assert row_bytes % u == 0 and src % u == 0 and dst % u == 0
        signed = key_set - (1 << 64) if key_set >> 63 else key_set  # the table is int64 words
        self._item(_lib.SD_COMPACT, self.G * 64, SRC=src, DST=dst, SRC_PTR=src_ptr, DST_OFF=self.vector(dst_off), N=n, SRC_W=row_bytes // u,
                   DST_W=row_bytes // u, A0=key, A1=signed, UNIT=u)

    def rows_zero(self, src: int, dst: int, src_ptr: int, dst_off, n: int, row_bytes: int, key: int, key_set: int):
        """rows copied, written as zeros where the row's int64 ``key`` is in the 64-bit ``key_set``"""
        assert 0 <= key_set < 1 << 64
        if n == 0 or row_bytes == 0:
            return
        u = _unit_of(row_bytes, src, dst)
        signed = key_set - (1 << 64) if key_set >> 63 else key_set
        self._item(_lib.SD_ROWS_ZERO, n * (row_bytes // u), SRC=src, DST=dst, SRC_PTR=src_ptr, DST_OFF=self.vector(dst_off), N=n,
                   SRC_W=row_bytes // u, TAKE=row_bytes // u, DST_W=row_bytes // u, A0=key, A1=signed, UNIT=u)

    def layout(self):
        """``(words, item_word0, vector_word0 [n_vectors])`` of the block: group table (even count), items, vectors (16-byte aligned)"""
        n = len(self.items)
        n_groups = (n + 63) // 64
        item0 = (n_groups + 1) & ~1
        pos = item0 + n * _lib.SD_ITEM_WORDS
        where = []
        for v in self.vectors:
            where.append(pos)
            pos += (v.size + 1) & ~1
        return pos, item0, where

    def pack(self, base_addr: int):
        """``(block int64 [words], n_blocks)`` for a block that will live at device address ``base_addr``"""
        n = len(self.items)
        if n > _lib.SD_MAX_ITEMS:
            raise _lib.HydraMPError(f"the derive launch would run {n} items, its group table holds {_lib.SD_MAX_ITEMS}")
        words, item0, where = self.layout()
        block = np.zeros(max(words, 2), dtype=np.int64)
        blocks = 0
        for i, (it, w) in enumerate(zip(self.items, self.work)):
            row = [base_addr + 8 * where[v[1]] if isinstance(v, tuple) else v for v in it]
            row[_lib.SD_BLOCK0] = blocks
            block[item0 + i * _lib.SD_ITEM_WORDS: item0 + (i + 1) * _lib.SD_ITEM_WORDS] = row
            if i % 64 == 0:
                block[i // 64] = blocks
            blocks += min((w + self.THREADS - 1) // self.THREADS, self.MAX_BLOCKS)
        for v, p in zip(self.vectors, where):
            block[p:p + v.size] = v
        return block, blocks


def _run_plan(store: "GraphStore", plan: DerivePlan, keep: Sequence[np.ndarray] = ()):
    """upload the plan's block (one copy) and launch; ``keep``: offset vectors the result needs on the device -- they travel in the
    same block and come back as views of it"""
    handles = [plan.vector(v) for v in keep]
    words, _, where = plan.layout()
    dev = torch.empty(max(words, 2), dtype=torch.int64, device=store.device)
    block, n_blocks = plan.pack(dev.data_ptr())
    dev.copy_(torch.from_numpy(block), non_blocking=False)
    _lib.check(store.lib.hmp_store_derive(dev.data_ptr(), len(plan.items), n_blocks, store.n_graphs, _lib.stream_ptr()))
    return [dev[where[h[1]]: where[h[1]] + plan.vectors[h[1]].size] for h in handles]


def _derived(self: "GraphStore") -> "GraphStore":
    """a store that shares every array with ``self`` (the containers are its own)"""
    new = object.__new__(GraphStore)
    new.device, new.lib, new.n_graphs, new.homogeneous = self.device, self.lib, self.n_graphs, self.homogeneous
    new._stage = new._stage_dev = new._copied = None
    new.node_types, new.edge_types = list(self.node_types), list(self.edge_types)
    new.node_counts, new.count_only = dict(self.node_counts), dict(self.count_only)
    new.node_attrs = {t: dict(a) for t, a in self.node_attrs.items()}
    new.edge_index, new.edge_ptr, new.edge_ptr_host = dict(self.edge_index), dict(self.edge_ptr), dict(self.edge_ptr_host)
    new.edge_rows = {e: dict(r) for e, r in self.edge_rows.items()}
    new.edge_attr = {e: new.edge_rows[e]["edge_attr"] for e in self.edge_attr}
    if self.homogeneous:
        new.homo_keys, new.edge_name = list(self.homo_keys), dict(self.edge_name)
    return new


def _own_masks(new: "GraphStore", plan: DerivePlan) -> None:
    """a derived store never shares mask rows with its parent (a later node split rewrites them in place): copy them in the launch"""
    for t, attrs in new.node_attrs.items():
        for k in DEFAULT_MASKS:
            pk = attrs.get(k)
            if pk is None:
                continue
            out = _derive_alloc(tuple(pk.data.shape), pk.data.dtype, new.device)
            plan.rows(pk.data.data_ptr(), out.data_ptr(), pk.ptr.data_ptr(), pk.ptr_host[:-1], int(pk.ptr_host[-1]), pk.row_bytes, 0,
                      pk.row_bytes, pk.row_bytes)
            attrs[k] = _packed(out, pk.ptr, pk.ptr_host)


def _features(self: "GraphStore", t: str, what: str) -> _Packed:
    pk = self.node_attrs[t].get("x")
    if pk is None:
        raise _lib.HydraMPError(f"{what}: node type '{t}' has no features 'x'")
    if pk.data.dtype != torch.float32 or pk.data.dim() != 2:
        raise _lib.HydraMPError(f"{what}: 'x' of node type '{t}' must be a float32 matrix, the store holds {tuple(pk.data.shape[1:])} {pk.data.dtype}")
    return pk


def _narrow_x(self: "GraphStore", new: "GraphStore", plan: DerivePlan, t: str, pk: _Packed, skip: int, take: int) -> None:
    n = int(pk.ptr_host[-1])
    out = _derive_alloc((n, take), torch.float32, self.device)
    plan.rows(pk.data.data_ptr(), out.data_ptr(), pk.ptr.data_ptr(), pk.ptr_host[:-1], n, pk.row_bytes, 4 * skip, 4 * take, 4 * take)
    new.node_attrs[t]["x"] = _packed(out, pk.ptr, pk.ptr_host)


def _with_relative_pos(self: "GraphStore") -> "GraphStore":
    """The store of ``data.compute_relative_pos`` applied to every graph (reference ``mp3d_dataset.py:298-319``): every ``x`` loses its
    three leading position columns and every edge type gains ``edge_attr = pos_dst[ei[1]] - pos_src[ei[0]]``.  A new store; the
    receiver is unchanged and shares the arrays that do not change."""
    what = "with_relative_pos"
    if self.homogeneous:
        raise _lib.HydraMPError(f"{what}: works on a typed store (derive the homogeneous one afterwards: .to_homogeneous())")
    if self.edge_attr:
        raise _lib.HydraMPError(f"{what}: the store already holds 'edge_attr' ({list(self.edge_attr)[0]})")
    xs = {t: _features(self, t, what) for t in self.node_types}
    for t, pk in xs.items():
        if pk.data.size(1) < 3:
            raise _lib.HydraMPError(f"{what}: 'x' of node type '{t}' is {pk.data.size(1)} wide, narrower than the 3 position columns")
    pos = {}
    for e in self.edge_types:
        for t in (e[0], e[2]):
            pk = self.node_attrs.get(t, {}).get("pos")
            if pk is None:
                raise _lib.HydraMPError(f"{what}: node type '{t}' (an end of {e}) has no positions 'pos'")
            if pk.data.dtype != torch.float32 or pk.row_shape != (3,):
                raise _lib.HydraMPError(f"{what}: 'pos' of node type '{t}' must be float32 [n, 3], the store holds {pk.row_shape} {pk.data.dtype}")
            pos[t] = pk
    new, plan = _derived(self), DerivePlan(self.n_graphs)
    for t, pk in xs.items():
        _narrow_x(self, new, plan, t, pk, 3, pk.data.size(1) - 3)
    for e in self.edge_types:
        ei = self.edge_index[e]
        n = int(ei.size(1))
        out = _derive_alloc((n, 3), torch.float32, self.device)
        plan.relpos(ei.data_ptr(), out.data_ptr(), self.edge_ptr[e].data_ptr(), n, pos[e[0]].data.data_ptr(), pos[e[2]].data.data_ptr(),
                    pos[e[0]].ptr.data_ptr(), pos[e[2]].ptr.data_ptr())
        pk = _packed(out, self.edge_ptr[e], self.edge_ptr_host[e])
        new.edge_attr[e] = pk
        new.edge_rows[e] = {"edge_attr": pk}
    _own_masks(new, plan)
    _run_plan(self, plan)
    return new


def _remove_last_features(self: "GraphStore", dim: int) -> "GraphStore":
    """The store of the reference's ``remove_last_features(dim)`` (``mp3d_dataset.py:286-296``): every ``x`` at least ``dim`` wide loses
    its last ``dim`` columns, a narrower one is kept.  Typed and homogeneous stores."""
    what = "remove_last_features"
    dim = int(dim)
    if dim <= 0:
        raise _lib.HydraMPError(f"{what}: dim must be positive, got {dim}")
    new, plan = _derived(self), DerivePlan(self.n_graphs)
    for t in self.node_types:
        if "x" not in self.node_attrs[t]:
            continue
        pk = _features(self, t, what)
        if pk.data.size(1) >= dim:
            _narrow_x(self, new, plan, t, pk, 0, pk.data.size(1) - dim)
    _own_masks(new, plan)
    _run_plan(self, plan)
    return new


def _to_homogeneous(self: "GraphStore", removed_edge_type: Optional[EdgeType] = None) -> "GraphStore":
    """The homogeneous store of the same graphs.  Without ``object_virtual`` / ``room_virtual`` node types:
    ``data.heterogeneous_data_to_homogeneous`` per graph plus ``room_mask = node_type == index("rooms")``; with them:
    ``data.heterogeneous_htree_to_homogeneous`` (reference ``mp3d_dataset.py:29-119``).  Node types with ``x`` take part, in store order;
    features are zero-padded to the widest type.  ``removed_edge_type`` (a store without virtual node types only, as in the reference,
    ``mp3d_dataset.py:53-69``): the edges of that type stay out of ``edge_index`` / ``edge_type`` / ``edge_attr`` -- a change to the plan
    alone, the removed type contributes no item -- and the other types keep their numbers."""
    plan, parts = _plan_to_homogeneous(self, removed_edge_type)
    return _finish_to_homogeneous(self, plan, *parts)


def _plan_to_homogeneous(self: "GraphStore", removed_edge_type: Optional[EdgeType] = None):
    """the plan of ``to_homogeneous`` and what the new store is assembled from: every output is allocated, nothing is launched"""
    what = "to_homogeneous"
    if self.homogeneous:
        raise _lib.HydraMPError(f"{what}: the store is homogeneous already")
    types = [t for t in self.node_types if "x" in self.node_attrs[t]]
    if not types:
        raise _lib.HydraMPError(f"{what}: no node type has features 'x'")
    xs = {t: _features(self, t, what) for t in types}
    htree = "object_virtual" in types and "room_virtual" in types
    if not htree and "rooms" not in types:
        raise _lib.HydraMPError(f"{what}: no node type 'rooms' with features 'x' (room_mask marks its rows)")
    virtual = ("object_virtual", "room_virtual") if htree else ()
    if removed_edge_type is not None:
        removed_edge_type = tuple(removed_edge_type)
        if htree:
            raise _lib.HydraMPError(f"{what}: removed_edge_type is refused on an H-tree store (the reference's H-tree converter has no "
                                    f"such argument); on the homogeneous store: .without_edge_types([ids])")
        if removed_edge_type not in self.edge_types:
            raise _lib.HydraMPError(f"{what}: removed_edge_type {removed_edge_type} is not an edge type of the store: {self.edge_types}")
    group_of = {}
    for e in self.edge_types:
        for t in (e[0], e[2]):
            if t not in types:
                raise _lib.HydraMPError(f"{what}: edge type {e} touches node type '{t}', which has no features 'x'")
        if e[0] in virtual and e[2] in virtual:
            raise _lib.HydraMPError(f"{what}: edge type {e} has a virtual node type at both ends (it would be an init and a pool edge)")
        group_of[e] = "init_edge_index" if e[0] in virtual else "pool_edge_index" if e[2] in virtual else "edge_index"
    G, dev = self.n_graphs, self.device
    width = max(int(pk.data.size(1)) for pk in xs.values())
    # labels: every type has them, or (H-tree) room_virtual has them and the others are filled with -1
    ys = {t: self.node_attrs[t].get("y") for t in types}
    if htree and ys["room_virtual"] is not None:
        has_y = True
    else:
        has_y = all(v is not None for v in ys.values())
    if has_y:
        y0 = ys["room_virtual"] if htree else ys[types[0]]
        for t, pk in ys.items():
            if pk is not None and (pk.data.dtype != y0.data.dtype or pk.row_shape != ()):
                raise _lib.HydraMPError(f"{what}: 'y' of node type '{t}' is {pk.row_shape} {pk.data.dtype}, expected a {y0.data.dtype} vector")
        if any(v is None for v in ys.values()) and y0.data.dtype != torch.int64:
            raise _lib.HydraMPError(f"{what}: 'y' must be int64 for the -1 rows of the node types without labels, the store holds {y0.data.dtype}")
    has_ea = len(self.edge_types) > 0 and all(e in self.edge_attr for e in self.edge_types)
    if has_ea:
        ea0 = self.edge_attr[self.edge_types[0]]
        for e in self.edge_types:
            if self.edge_attr[e].row_shape != ea0.row_shape or self.edge_attr[e].data.dtype != ea0.data.dtype:
                raise _lib.HydraMPError(f"{what}: 'edge_attr' of {e} is {self.edge_attr[e].row_shape}, of {self.edge_types[0]} {ea0.row_shape}")

    plan = DerivePlan(G)
    node_ptr, inside, node_dst = plan_concat([self.node_counts[t] for t in types])
    N = int(node_ptr[-1])
    x = _derive_alloc((N, width), torch.float32, dev)
    node_type = _derive_alloc((N,), torch.int64, dev)
    y = _derive_alloc((N,), y0.data.dtype, dev) if has_y else None
    room_mask = _derive_alloc((N,), torch.bool, dev)
    object_mask = _derive_alloc((N,), torch.bool, dev) if htree else None
    room_type = "room_virtual" if htree else "rooms"
    for i, t in enumerate(types):
        pk = xs[t]
        n = int(pk.ptr_host[-1])
        assert np.array_equal(pk.counts, self.node_counts[t])
        cp = pk.ptr.data_ptr()
        plan.rows(pk.data.data_ptr(), x.data_ptr(), cp, node_dst[i], n, pk.row_bytes, 0, pk.row_bytes, 4 * width)
        plan.fill(node_type.data_ptr(), cp, node_dst[i], n, i, 8)
        if has_y and ys[t] is not None:
            plan.rows(ys[t].data.data_ptr(), y.data_ptr(), ys[t].ptr.data_ptr(), node_dst[i], n, ys[t].row_bytes, 0, ys[t].row_bytes, ys[t].row_bytes)
        elif has_y:
            plan.fill(y.data_ptr(), cp, node_dst[i], n, -1, 8)
        plan.fill(room_mask.data_ptr(), cp, node_dst[i], n, int(t == room_type), 1)
        if htree:
            plan.fill(object_mask.data_ptr(), cp, node_dst[i], n, int(t == "object_virtual"), 1)
    groups = ["edge_index"] + (["init_edge_index", "pool_edge_index"] if htree else [])
    edge_out, edge_ptr_host = {}, {}
    edge_type = edge_attr = None
    for name in groups:
        members = [e for e in self.edge_types if group_of[e] == name and e != removed_edge_type]
        if members:
            eptr, _, edst = plan_concat([np.diff(self.edge_ptr_host[e]) for e in members])
        else:
            eptr, edst = np.zeros(G + 1, dtype=np.int64), None
        E = int(eptr[-1])
        out = _derive_alloc((2, E), torch.int64, dev)
        edge_out[name], edge_ptr_host[name] = out, eptr
        if name == "edge_index":
            edge_type = _derive_alloc((E,), torch.int64, dev)
            if has_ea:
                edge_attr = _derive_alloc((E,) + ea0.row_shape, ea0.data.dtype, dev)
        for j, e in enumerate(members):
            n = int(self.edge_ptr_host[e][-1])
            ep = self.edge_ptr[e].data_ptr()
            plan.edges(self.edge_index[e].data_ptr(), out.data_ptr(), ep, edst[j], n, inside[types.index(e[0])], inside[types.index(e[2])], E)
            if name == "edge_index":
                plan.fill(edge_type.data_ptr(), ep, edst[j], n, self.edge_types.index(e), 8)
                if has_ea:
                    pk = self.edge_attr[e]
                    plan.rows(pk.data.data_ptr(), edge_attr.data_ptr(), ep, edst[j], n, pk.row_bytes, 0, pk.row_bytes, pk.row_bytes)
    return plan, (groups, node_ptr, edge_ptr_host, edge_out, edge_type, edge_attr, x, node_type, y, room_mask, object_mask, has_y, has_ea,
                  htree)


def _finish_to_homogeneous(self, plan, groups, node_ptr, edge_ptr_host, edge_out, edge_type, edge_attr, x, node_type, y, room_mask, object_mask,
                           has_y, has_ea, htree) -> "GraphStore":
    G, dev = self.n_graphs, self.device
    dev_vecs = _run_plan(self, plan, keep=[node_ptr] + [edge_ptr_host[name] for name in groups])
    node_ptr_dev, edge_ptr_dev = dev_vecs[0], dict(zip(groups, dev_vecs[1:]))

    new = object.__new__(GraphStore)
    new.device, new.lib, new.n_graphs, new.homogeneous = dev, self.lib, G, True
    new._stage = new._stage_dev = new._copied = None
    new.homo_keys = (["x", "node_type", "edge_index", "edge_type"] + (["y"] if has_y else []) + (["edge_attr"] if has_ea else [])
                     + groups[1:] + ["room_mask"] + (["object_mask"] if htree else []))
    new.node_types, new.node_counts, new.count_only = [HOMO_NODE], {HOMO_NODE: np.diff(node_ptr)}, {HOMO_NODE: False}
    arrays = {"x": x, "node_type": node_type, "y": y, "room_mask": room_mask, "object_mask": object_mask}
    new.node_attrs = {HOMO_NODE: {k: _packed(arrays[k], node_ptr_dev, node_ptr) for k in new.homo_keys if k in arrays}}
    new.edge_types, new.edge_name = [], {}
    new.edge_index, new.edge_ptr, new.edge_ptr_host, new.edge_attr, new.edge_rows = {}, {}, {}, {}, {}
    for name in groups:
        e = homo_edge_type(name)
        new.edge_types.append(e)
        new.edge_name[e] = name
        new.edge_index[e], new.edge_ptr[e], new.edge_ptr_host[e] = edge_out[name], edge_ptr_dev[name], edge_ptr_host[name]
    e0 = homo_edge_type("edge_index")
    new.edge_rows[e0] = {"edge_type": _packed(edge_type, new.edge_ptr[e0], new.edge_ptr_host[e0])}
    if has_ea:
        new.edge_attr[e0] = new.edge_rows[e0]["edge_attr"] = _packed(edge_attr, new.edge_ptr[e0], new.edge_ptr_host[e0])
    return new


def _empty_packed(pk: _Packed, ptr: torch.Tensor, ptr_host: np.ndarray) -> _Packed:
    return _packed(torch.empty((0,) + pk.row_shape, dtype=pk.data.dtype, device=pk.data.device), ptr, ptr_host)


def _without_edge_types(self: "GraphStore", edge_types) -> "GraphStore":
    """The store of ``data.remove_edge_types`` applied to every graph.  Typed store: ``edge_types`` are triples; each stays in the store
    with no edge in any graph (the reference's ``noRE`` data, ``remove_room_edges_in_dsg``, for ``rooms_to_rooms``) -- nothing but the mask
    rows is copied.  Homogeneous store: ``edge_types`` are ints below 64; the columns of ``edge_index`` with that ``edge_type`` are
    dropped, ``edge_type`` and ``edge_attr`` follow, ``init_edge_index`` / ``pool_edge_index`` stay: a count launch
    (``hmp_store_count_kept``), one read of ``G`` int64, and a stable compaction in the derive launch."""
    what = "without_edge_types"
    edge_types = list(edge_types)
    new, plan = _derived(self), DerivePlan(self.n_graphs)
    G, dev = self.n_graphs, self.device
    if not self.homogeneous:
        for e in edge_types:
            if not isinstance(e, (tuple, list)) or tuple(e) not in self.edge_types:
                raise _lib.HydraMPError(f"{what}: {e!r} is not an edge type of the store: {self.edge_types}")
        zero_host = np.zeros(G + 1, dtype=np.int64)
        zero_dev = torch.zeros(G + 1, dtype=torch.int64, device=dev)
        for e in dict.fromkeys(tuple(e) for e in edge_types):
            new.edge_index[e] = torch.empty((2, 0), dtype=torch.int64, device=dev)
            new.edge_ptr[e], new.edge_ptr_host[e] = zero_dev, zero_host
            if e in new.edge_rows:
                new.edge_rows[e] = {k: _empty_packed(pk, zero_dev, zero_host) for k, pk in self.edge_rows[e].items()}
            if e in new.edge_attr:
                new.edge_attr[e] = new.edge_rows[e]["edge_attr"]
        _own_masks(new, plan)
        if plan.items:
            _run_plan(self, plan)
        return new
    ids = []
    for t in edge_types:
        if isinstance(t, (bool, tuple, list, str)) or int(t) != t:
            raise _lib.HydraMPError(f"{what}: a homogeneous store takes edge type numbers (ints), got {t!r}")
        if not 0 <= int(t) < 64:
            raise _lib.HydraMPError(f"{what}: edge type number {int(t)} is outside [0, 64): the removed types travel as a 64-bit set")
        ids.append(int(t))
    e0 = homo_edge_type("edge_index")
    rows = self.edge_rows.get(e0, {})
    if e0 not in self.edge_index or "edge_type" not in rows:
        raise _lib.HydraMPError(f"{what}: the store holds no 'edge_type' rows of 'edge_index'")
    key = rows["edge_type"]
    if key.data.dtype != torch.int64 or key.row_shape != ():
        raise _lib.HydraMPError(f"{what}: 'edge_type' must be an int64 vector, the store holds {key.row_shape} {key.data.dtype}")
    key_set = 0
    for t in ids:
        key_set |= 1 << t
    ei, ep, ep_host = self.edge_index[e0], self.edge_ptr[e0], self.edge_ptr_host[e0]
    E = int(ep_host[-1])
    kept = torch.empty(G, dtype=torch.int64, device=dev)
    _lib.check(self.lib.hmp_store_count_kept(key.data.data_ptr() if E else None, ep.data_ptr(), G, key_set, kept.data_ptr(), _lib.stream_ptr()))
    counts = kept.cpu().numpy()  # the one device-to-host read: G int64
    ptr_host = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    E_new = int(ptr_host[-1])
    out_ei = _derive_alloc((2, E_new), torch.int64, dev)
    kp, sp = key.data.data_ptr(), ep.data_ptr()
    if E_new:
        for r in range(2):
            plan.compact(ei.data_ptr() + 8 * E * r, out_ei.data_ptr() + 8 * E_new * r, sp, ptr_host[:-1], E, 8, kp, key_set)
    out_rows = {}
    for k, pk in rows.items():
        out_rows[k] = _derive_alloc((E_new,) + pk.row_shape, pk.data.dtype, dev)
        if pk.row_bytes % 4:
            raise _lib.HydraMPError(f"{what}: '{k}' rows of {pk.row_bytes} bytes (the compaction moves 4- or 8-byte units)")
        if E_new:
            plan.compact(pk.data.data_ptr(), out_rows[k].data_ptr(), sp, ptr_host[:-1], E, pk.row_bytes, kp, key_set)
    _own_masks(new, plan)
    (ptr_dev,) = _run_plan(self, plan, keep=[ptr_host])
    new.edge_index[e0], new.edge_ptr[e0], new.edge_ptr_host[e0] = out_ei, ptr_dev, ptr_host
    new.edge_rows[e0] = {k: _packed(v, ptr_dev, ptr_host) for k, v in out_rows.items()}
    if e0 in self.edge_attr:
        new.edge_attr[e0] = new.edge_rows[e0]["edge_attr"]
    return new


CLIQUE_NODE_TYPES = ("object-room", "room-room")


def _zero_clique_features(self: "GraphStore") -> "GraphStore":
    """The store of ``data.zero_clique_features`` applied to every graph (reference ``train_Stanford.py:93-99``): ``x`` of the two clique
    node types of an H-tree is zero.  Typed store: the two types' ``x``; homogeneous H-tree store: the rows of ``x`` whose ``node_type`` is
    one of the two.  A store that is not an H-tree is refused."""
    what = "zero_clique_features"
    new, plan = _derived(self), DerivePlan(self.n_graphs)
    if not self.homogeneous:
        for t in CLIQUE_NODE_TYPES:
            if t not in self.node_types or "x" not in self.node_attrs[t]:
                raise _lib.HydraMPError(f"{what}: the store holds no node type '{t}' with features 'x' (not an H-tree store)")
        for t in CLIQUE_NODE_TYPES:
            pk = _features(self, t, what)
            n = int(pk.ptr_host[-1])
            out = _derive_alloc(tuple(pk.data.shape), torch.float32, self.device)
            plan.rows(pk.data.data_ptr(), out.data_ptr(), pk.ptr.data_ptr(), pk.ptr_host[:-1], n, pk.row_bytes, 0, 0, pk.row_bytes)
            new.node_attrs[t]["x"] = _packed(out, pk.ptr, pk.ptr_host)
    else:
        attrs = self.node_attrs[HOMO_NODE]
        if "object_mask" not in attrs or "node_type" not in attrs:
            raise _lib.HydraMPError(f"{what}: the homogeneous store is not an H-tree store (no 'object_mask' / 'node_type')")
        pk, key = _features(self, HOMO_NODE, what), attrs["node_type"]
        if key.data.dtype != torch.int64 or key.row_shape != ():
            raise _lib.HydraMPError(f"{what}: 'node_type' must be an int64 vector, the store holds {key.row_shape} {key.data.dtype}")
        from .data import HTREE_NODE_TYPES
        key_set = 0
        for t in CLIQUE_NODE_TYPES:
            key_set |= 1 << HTREE_NODE_TYPES.index(t)
        n = int(pk.ptr_host[-1])
        out = _derive_alloc(tuple(pk.data.shape), torch.float32, self.device)
        plan.rows_zero(pk.data.data_ptr(), out.data_ptr(), pk.ptr.data_ptr(), pk.ptr_host[:-1], n, pk.row_bytes, key.data.data_ptr(), key_set)
        new.node_attrs[HOMO_NODE]["x"] = _packed(out, pk.ptr, pk.ptr_host)
    _own_masks(new, plan)
    if plan.items:
        _run_plan(self, plan)
    return new


# ---- node split -----------------------------------------------------------------------------------------------------------
def node_split_assignment(total: int, ratios, seed: int = 0) -> np.ndarray:
    """The shuffled assignment list of the reference's ``generate_node_split`` (``Stanford3DSG_dataset.py:462-492``) as an int8
    vector: 1 train, 2 val, 3 test, 0 unassigned (ratios that sum to less than 1).  ``ratios = (train, val, test)``, ``test`` may be
    None (= the rest).  The stdlib ``random`` in the reference's order of calls: exact by construction."""
    import random

    train, val, test = ratios
    random.seed(seed)
    assert train > 0
    assert val >= 0
    if test is None:
        test = 1 - train - val
    assert test >= 0
    assert train + val + test <= 1
    total = int(total)
    n_train, n_val = round(total * train), round(total * val)
    if train + val + test == 1:
        n_test = total - n_train - n_val
        out = [1] * n_train + [2] * n_val + [3] * n_test
    else:
        n_test = round(total * test)
        out = [1] * n_train + [2] * n_val + [3] * n_test + [0] * (total - n_train - n_val - n_test)
    random.shuffle(out)
    if len(out) != total:
        raise _lib.HydraMPError(f"node split: the ratios {tuple(ratios)} assign {len(out)} of {total} nodes")
    return np.array(out, dtype=np.int8)


def _split_layout(self: "GraphStore"):
    """``(data type, parts)`` of the reference's ``data_type()``: the node types whose rows a split assigns, in its order"""
    if self.homogeneous:
        attrs = self.node_attrs[HOMO_NODE]
        return ("homogeneous_htree" if "object_mask" in attrs and "room_mask" in attrs else "homogeneous"), [HOMO_NODE]
    if "object_virtual" in self.node_types and "room_virtual" in self.node_types:
        return "heterogeneous_htree", ["object_virtual", "room_virtual"]
    for t in ("objects", "rooms"):
        if t not in self.node_types:
            raise _lib.HydraMPError(f"generate_node_split: the store holds no node type '{t}'")
    return "heterogeneous", ["objects", "rooms"]


def _generate_node_split(self: "GraphStore", train_node_ratio, val_node_ratio, test_node_ratio, seed=0) -> None:
    """``Stanford3DSG_dataset.generate_node_split`` (reference ``:459-578``) on the resident store: ``train_mask`` / ``val_mask`` /
    ``test_mask`` of the node types the data type splits, written by one launch from one uploaded assignment vector.  The first call
    allocates the mask rows; later calls rewrite them in place, so an open stream's next batch carries the new split."""
    G, dev, lib = self.n_graphs, self.device, self.lib
    kind, parts = _split_layout(self)
    state = self.__dict__.setdefault("_split", {})
    if "ptr" not in state:  # [G + 1] row offsets of the parts on the device, and the members per graph
        state["ptr"] = {}
        for t in parts:
            any_pk = next(iter(self.node_attrs[t].values()), None)
            host = np.concatenate([[0], np.cumsum(self.node_counts[t])]).astype(np.int64)
            state["ptr"][t] = (any_pk.ptr if any_pk is not None else torch.from_numpy(host).to(dev), host)
        if kind == "homogeneous_htree":
            attrs = self.node_attrs[HOMO_NODE]
            for k in ("object_mask", "room_mask"):
                if attrs[k].data.dtype != torch.bool or attrs[k].row_shape != ():
                    raise _lib.HydraMPError(f"generate_node_split: '{k}' must be a bool vector, the store holds {attrs[k].row_shape} {attrs[k].data.dtype}")
            counts = torch.empty((2, G), dtype=torch.int64, device=dev)
            _lib.check(lib.hmp_store_member_counts(attrs["object_mask"].data.data_ptr(), attrs["room_mask"].data.data_ptr(),
                                                   state["ptr"][HOMO_NODE][0].data_ptr(), G, counts.data_ptr(), _lib.stream_ptr()))
            state["members"] = counts.cpu().numpy().sum(axis=0)  # the one device-to-host read, on the first call
        else:
            state["members"] = np.sum([self.node_counts[t] for t in parts], axis=0).astype(np.int64)
    members = state["members"]
    assign = node_split_assignment(int(members.sum()), (train_node_ratio, val_node_ratio, test_node_ratio), seed)
    off = np.concatenate([[0], np.cumsum(members)]).astype(np.int64)
    buf = np.concatenate([off.view(np.uint8), assign.view(np.uint8), np.zeros(1, dtype=np.uint8)])
    block = torch.from_numpy(buf).to(dev)  # one upload: [G + 1] offsets, then the assignments
    rows = []
    for t in parts:
        attrs = self.node_attrs[t]
        ptr_dev, ptr_host = state["ptr"][t]
        for k in DEFAULT_MASKS:
            pk = attrs.get(k)
            if pk is None:
                pk = attrs[k] = _packed(_derive_alloc((int(ptr_host[-1]),), torch.bool, dev), ptr_dev, ptr_host)
                if self.homogeneous:
                    self.homo_keys.append(k)
            elif pk.data.dtype != torch.bool or pk.row_shape != ():
                raise _lib.HydraMPError(f"generate_node_split: '{k}' of node type '{t}' must be a bool vector, the store holds "
                                        f"{pk.row_shape} {pk.data.dtype}")
            rows.append(pk.data.data_ptr())
    rows += [None] * (6 - len(rows))
    ranked = kind == "homogeneous_htree"
    attrs = self.node_attrs[parts[0]]
    _lib.check(lib.hmp_store_node_split(block.data_ptr() + 8 * (G + 1), block.data_ptr(), G, state["ptr"][parts[0]][0].data_ptr(),
                                        state["ptr"][parts[1]][0].data_ptr() if len(parts) > 1 else None,
                                        attrs["object_mask"].data.data_ptr() if ranked else None,
                                        attrs["room_mask"].data.data_ptr() if ranked else None, *rows, _lib.stream_ptr()))


GraphStore.with_relative_pos = _with_relative_pos
GraphStore.to_homogeneous = _to_homogeneous
GraphStore.remove_last_features = _remove_last_features
GraphStore.without_edge_types = _without_edge_types
GraphStore.zero_clique_features = _zero_clique_features
GraphStore.generate_node_split = _generate_node_split
GraphStore.__len__ = lambda self: self.n_graphs


class _StoreDatasetInfo:
    """what the jobs read from ``dataset.get_data(0)``"""

    def __init__(self, num_node_features, num_room_labels, num_object_labels):
        self._f, self._r, self._o = num_node_features, num_room_labels, num_object_labels

    def num_node_features(self):
        return self._f

    def num_room_labels(self):
        return self._r

    def num_object_labels(self):
        return self._o


class StoreDataset:
    """A resident :class:`GraphStore` under the interface of the reference's dataset containers as far as the training jobs read
    them (``jobs.py``): ``len``, ``data_type()``, ``get_data(0)`` with the three dimension accessors, ``generate_node_split``.  The jobs
    use the store as it is -- no host graphs in between.  ``num_node_features``: an int (homogeneous) or a dict per node type."""

    def __init__(self, store: GraphStore, data_type: str, num_node_features, num_room_labels: int, num_object_labels: Optional[int] = None):
        if data_type not in ("homogeneous", "heterogeneous", "homogeneous_htree", "heterogeneous_htree"):
            raise _lib.HydraMPError(f"StoreDataset: unknown data type '{data_type}'")
        if (data_type.split("_")[0] == "homogeneous") != store.homogeneous:
            raise _lib.HydraMPError(f"StoreDataset: data type '{data_type}' for a {'homogeneous' if store.homogeneous else 'typed'} store")
        self.store, self._data_type = store, data_type
        self._info = _StoreDatasetInfo(num_node_features, num_room_labels, num_object_labels)

    def __len__(self):
        return self.store.n_graphs

    def __getitem__(self, i):
        raise _lib.HydraMPError("a StoreDataset holds no host graphs: batches come from its store (store.collate / store.stream)")

    def data_type(self):
        return self._data_type

    def get_data(self, i):
        return self._info

    def generate_node_split(self, train_node_ratio, val_node_ratio, test_node_ratio, seed=0):
        self.store.generate_node_split(train_node_ratio, val_node_ratio, test_node_ratio, seed=seed)
