"""Seeded synthetic scene-graph workloads for the BASELINE.json configs.

Real MP3D trajectory graphs and the word2vec table are not available offline, so the bench and the
parity tests use MP3D-*shaped* graphs: same node/edge types (reference
``src/hydra_gnn/mp3d_dataset.py:21-26``), same feature contract (objects 306-d =
pos(3) | bbox size(3) | semantic(300); rooms 6-d; 26 room labels with 25 = ignored,
``src/hydra_gnn/base_training_job.py:63``), statistics taken from the one real fixture graph
(5 rooms / 62 objects, mean object in-degree 5.74).

Everything is generated with ``numpy.random.Generator(PCG64(seed))`` so the same seed gives the
same graphs here and on the GPU box.
"""
from __future__ import annotations

import os
from typing import List, Optional

import numpy as np
import torch

from .data import EDGE_TYPES, Data, HeteroData, collate, compute_relative_pos

BASE_SEED = 20250225
NUM_ROOM_LABELS = 26
IGNORED_LABEL = 25


def _sym_edges(pairs: np.ndarray) -> np.ndarray:
    """undirected pairs [M,2] -> directed edge_index [2, 2M] with both directions (u->v then v->u)."""
    if pairs.size == 0:
        return np.zeros((2, 0), dtype=np.int64)
    return np.concatenate([pairs.T, pairs[:, ::-1].T], axis=1).astype(np.int64)


def mp3d_like_graph(rng: np.random.Generator, sem_dim: int = 300, mean_in_degree: float = 6.0) -> HeteroData:
    n_rooms = int(rng.integers(2, 13))
    per_room = np.maximum(rng.poisson(12.0, size=n_rooms), 1)
    n_obj = int(per_room.sum())
    room_of = np.repeat(np.arange(n_rooms), per_room)
    obj_start = np.concatenate([[0], np.cumsum(per_room)])

    # objects <-> objects: within-room undirected pairs, expected in-degree ~ mean_in_degree
    pairs = []
    for r in range(n_rooms):
        k = int(per_room[r])
        if k < 2:
            continue
        n_pairs_all = k * (k - 1) // 2
        want = min(n_pairs_all, int(round(mean_in_degree * k / 2.0)))
        iu, ju = np.triu_indices(k, 1)
        sel = rng.choice(n_pairs_all, size=want, replace=False)
        sel.sort()
        pairs.append(np.stack([iu[sel], ju[sel]], 1) + obj_start[r])
    oo = _sym_edges(np.concatenate(pairs, 0) if pairs else np.zeros((0, 2), dtype=np.int64))

    # rooms <-> rooms: random spanning tree + 20 % extra undirected edges
    tree = np.array([[int(rng.integers(0, v)), v] for v in range(1, n_rooms)], dtype=np.int64).reshape(-1, 2)
    extra_n = int(round(0.2 * max(n_rooms - 1, 0)))
    have = {(int(a), int(b)) for a, b in tree}
    extra = []
    tries = 0
    while len(extra) < extra_n and tries < 50:
        tries += 1
        a, b = sorted(int(v) for v in rng.choice(n_rooms, size=2, replace=False))
        if (a, b) not in have:
            have.add((a, b))
            extra.append([a, b])
    rr_pairs = np.concatenate([tree, np.array(extra, dtype=np.int64).reshape(-1, 2)], 0)
    rr = _sym_edges(rr_pairs)

    # rooms -> objects: one edge per object; objects -> rooms is the flipped copy
    # (reference src/hydra_gnn/mp3d_dataset.py:247-249)
    ro = np.stack([room_of, np.arange(n_obj)], 0).astype(np.int64)

    def feats(n, with_sem):
        pos = rng.normal(0.0, 5.0, size=(n, 3))
        size = rng.uniform(0.1, 2.0, size=(n, 3))
        cols = [pos, size]
        if with_sem and sem_dim > 0:
            cols.append(rng.normal(0.0, 0.15, size=(n, sem_dim)))
        return np.concatenate(cols, 1).astype(np.float32), pos.astype(np.float32)

    xo, po = feats(n_obj, True)
    xr, pr = feats(n_rooms, False)

    g = HeteroData()
    g["objects"].x = torch.from_numpy(xo)
    g["objects"].pos = torch.from_numpy(po)
    g["objects"].y = torch.from_numpy(rng.integers(0, 28, size=n_obj).astype(np.int64))
    g["rooms"].x = torch.from_numpy(xr)
    g["rooms"].pos = torch.from_numpy(pr)
    g["rooms"].y = torch.from_numpy(rng.integers(0, NUM_ROOM_LABELS, size=n_rooms).astype(np.int64))
    g["objects", "objects_to_objects", "objects"].edge_index = torch.from_numpy(oo)
    g["rooms", "rooms_to_rooms", "rooms"].edge_index = torch.from_numpy(rr)
    g["objects", "objects_to_rooms", "rooms"].edge_index = torch.from_numpy(ro[::-1].copy())
    g["rooms", "rooms_to_objects", "objects"].edge_index = torch.from_numpy(ro)
    return g


def mp3d_like_batch(batch_size: int, seed: int, relative_pos: bool = False, sem_dim: int = 300) -> HeteroData:
    """Config 2 (``seed = BASE_SEED + 2``, B=32) and config 3 (``BASE_SEED + 3``, B=64)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    graphs = [mp3d_like_graph(rng, sem_dim=sem_dim) for _ in range(batch_size)]
    if relative_pos:
        for g in graphs:
            compute_relative_pos(g)
    return collate(graphs)


def semisupervised_batch(n_graphs: int, seed: int, relative_pos: bool = False) -> HeteroData:
    """Batch of the two-headed (room + object) task, ``SemiSupervisedTrainingJob`` (semisupervised_training_job.py:117-147):
    ``mp3d_like_graph`` graphs (room labels 0..25, object labels 0..27; no label is ignored) with a seeded per-node split of
    BOTH node types into disjoint ``train_mask`` (60 %), ``val_mask`` (20 %) and ``test_mask`` (20 %) bool tensors."""
    rng = np.random.Generator(np.random.PCG64(seed))
    graphs = [mp3d_like_graph(rng) for _ in range(n_graphs)]
    if relative_pos:
        for g in graphs:
            compute_relative_pos(g)
    batch = collate(graphs)
    for t in ("rooms", "objects"):
        u = torch.from_numpy(rng.random(int(batch[t].y.numel())))
        batch[t].train_mask = u < 0.6
        batch[t].val_mask = (u >= 0.6) & (u < 0.8)
        batch[t].test_mask = u >= 0.8
    return batch


def stanford_semisupervised_batch(n_graphs: int, seed: int) -> Data:
    """Batch of the homogeneous two-headed task (Stanford3DSG, ``SemiSupervisedTrainingJob`` with ``HomogeneousNetwork``):
    ``stanford_like_graph``s (room node 0 with a label in 0..14, objects 0..34), collated like PyG, with a seeded per-node split
    into disjoint ``train_mask`` (60 %), ``val_mask`` (20 %) and ``test_mask`` (20 %) bool tensors."""
    from .data import collate_homogeneous

    rng = np.random.Generator(np.random.PCG64(seed))
    batch = collate_homogeneous([stanford_like_graph(rng) for _ in range(n_graphs)])
    u = torch.from_numpy(rng.random(int(batch.y.numel())))
    batch.train_mask = u < 0.6
    batch.val_mask = (u >= 0.6) & (u < 0.8)
    batch.test_mask = u >= 0.8
    return batch


def config2_batch(batch_size: int = 32, rank: int = 0) -> HeteroData:
    return mp3d_like_batch(batch_size, BASE_SEED + 2 + 1000 * rank)


def config3_batch(batch_size: int = 64, rank: int = 0, edge: bool = False) -> HeteroData:
    return mp3d_like_batch(batch_size, BASE_SEED + 3 + 1000 * rank, relative_pos=edge)


def big_hetero_graph(n_obj: int = 1_000_000, n_rooms: int = 10_000, deg: int = 16, feat_dim: int = 256,
                     seed: int = BASE_SEED + 5, dtype=torch.float32) -> HeteroData:
    """Config 5: one large hetero graph (object in-neighbours 90 % own room / 10 % global)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    room_of = np.sort(rng.integers(0, n_rooms, size=n_obj)).astype(np.int64)
    start = np.searchsorted(room_of, np.arange(n_rooms), side="left")
    count = np.diff(np.concatenate([start, [n_obj]]))
    dst = np.repeat(np.arange(n_obj, dtype=np.int64), deg)
    local = rng.random(n_obj * deg) < 0.9
    r = room_of[dst]
    src_local = start[r] + (rng.random(n_obj * deg) * np.maximum(count[r], 1)).astype(np.int64)
    src_glob = rng.integers(0, n_obj, size=n_obj * deg)
    src = np.where(local, np.minimum(src_local, n_obj - 1), src_glob).astype(np.int64)
    oo = np.stack([src, dst], 0)
    ro = np.stack([room_of, np.arange(n_obj, dtype=np.int64)], 0)
    n_rr = 3 * n_rooms
    a = rng.integers(0, n_rooms, size=n_rr)
    b = rng.integers(0, n_rooms, size=n_rr)
    rr = _sym_edges(np.stack([a, b], 1))
    g = HeteroData()
    g["objects"].x = torch.from_numpy(rng.normal(0, 0.5, size=(n_obj, feat_dim)).astype(np.float32)).to(dtype)
    g["rooms"].x = torch.from_numpy(rng.normal(0, 0.5, size=(n_rooms, feat_dim)).astype(np.float32)).to(dtype)
    g["rooms"].y = torch.from_numpy(rng.integers(0, NUM_ROOM_LABELS, size=n_rooms).astype(np.int64))
    g["objects", "objects_to_objects", "objects"].edge_index = torch.from_numpy(oo)
    g["rooms", "rooms_to_rooms", "rooms"].edge_index = torch.from_numpy(rr)
    g["objects", "objects_to_rooms", "rooms"].edge_index = torch.from_numpy(ro[::-1].copy())
    g["rooms", "rooms_to_objects", "objects"].edge_index = torch.from_numpy(ro)
    g.num_graphs = 1
    return g


def stanford_like_graph(rng: np.random.Generator, n_nodes: Optional[int] = None) -> Data:
    """Config 1 input: a Stanford3DSG-shaped single-room graph (room is node 0, ``x`` is
    ``[N, 6]`` float32 = pos | size, N in 2..27, every object -> room in ONE direction, object <-> object symmetric,
    15 room / 35 object classes).  The reference's ``data/Stanford3DSG.pkl`` itself is not used: both
    ``torch.load(weights_only=True)`` and ``numpy.load(allow_pickle=False)`` refuse it."""
    n = int(n_nodes if n_nodes is not None else rng.integers(2, 28))
    x = np.concatenate([rng.normal(0, 3.0, size=(n, 3)), rng.uniform(0.1, 3.0, size=(n, 3))], 1).astype(np.float32)
    k = n - 1
    obj_room = np.stack([np.arange(1, n), np.zeros(k, dtype=np.int64)], 0)
    pairs = []
    if k >= 2:
        iu, ju = np.triu_indices(k, 1)
        want = min(len(iu), int(round(1.5 * k)))
        sel = np.sort(rng.choice(len(iu), size=want, replace=False))
        pairs = np.stack([iu[sel] + 1, ju[sel] + 1], 1)
    oo = _sym_edges(np.asarray(pairs, dtype=np.int64).reshape(-1, 2))
    y = np.concatenate([rng.integers(0, 15, size=1), rng.integers(0, 35, size=k)]).astype(np.int64)
    mask = np.zeros(n, dtype=bool)
    mask[0] = True
    return Data(x=torch.from_numpy(x), edge_index=torch.from_numpy(np.concatenate([obj_room, oo], 1).astype(np.int64)),
                y=torch.from_numpy(y), room_mask=torch.from_numpy(mask))


# ---------------------------------------------------------------------------------------------------------------------
# config 4: H-tree (Neural-Tree) batches from the committed topology fixture (tests/golden/htree_topologies.npz, made by
# tests/golden/make_htree_fixture.py with the reference's junction-tree code)
# ---------------------------------------------------------------------------------------------------------------------
from .data import HTREE_EDGE_TYPES, HTREE_INIT_EDGE_TYPES, HTREE_NODE_TYPES  # noqa: E402

HTREE_FIXTURE = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tests", "golden",
                             "htree_topologies.npz")


def htree_graph(npz, gi: int, rng: np.random.Generator) -> HeteroData:
    """One H-tree HeteroData (layout SURVEY Appendix B.2: object 306-d, room / object-room / room-room 6-d, ``room_virtual``
    carries ``num_nodes`` and ``y``; 10 message-passing edge types + the ``r_to_rv`` pool edges)."""
    counts = npz[f"g{gi}_counts"]
    n_rooms = int(npz[f"g{gi}_n_rooms"])
    g = HeteroData()
    dims = {"object": 306, "room": 6, "object-room": 6, "room-room": 6}
    for t, c in zip(HTREE_NODE_TYPES, counts):
        pos = rng.normal(0.0, 5.0, size=(int(c), 3))
        rest = rng.uniform(0.1, 2.0, size=(int(c), 3)) if t in ("object", "room") else np.zeros((int(c), 3))
        cols = [pos, rest]
        if dims[t] > 6:
            cols.append(rng.normal(0.0, 0.15, size=(int(c), dims[t] - 6)))
        g[t].x = torch.from_numpy(np.concatenate(cols, 1).astype(np.float32))
    for k, et in enumerate(HTREE_EDGE_TYPES):
        g[et].edge_index = torch.from_numpy(npz[f"g{gi}_e{k}"].astype(np.int64).reshape(2, -1))
    room_orig = npz[f"g{gi}_room_orig"].astype(np.int64)
    obj_orig = npz[f"g{gi}_object_orig"].astype(np.int64)
    n_objects = int(npz[f"g{gi}_n_objects"])
    g["room", "r_to_rv", "room_virtual"].edge_index = torch.from_numpy(np.stack([np.arange(len(room_orig)), room_orig], 0))
    g["object", "o_to_ov", "object_virtual"].edge_index = torch.from_numpy(np.stack([np.arange(len(obj_orig)), obj_orig], 0))
    # virtual nodes = copies of the original scene-graph nodes (construct.py:313-346): they carry x (read by pre_mp) and y
    g["room_virtual"].x = torch.from_numpy(np.concatenate([rng.normal(0.0, 5.0, size=(n_rooms, 3)),
                                                            rng.uniform(0.1, 2.0, size=(n_rooms, 3))], 1).astype(np.float32))
    g["object_virtual"].x = torch.from_numpy(np.concatenate([rng.normal(0.0, 5.0, size=(n_objects, 3)),
                                                              rng.uniform(0.1, 2.0, size=(n_objects, 3)),
                                                              rng.normal(0.0, 0.15, size=(n_objects, 300))], 1).astype(np.float32))
    g["room_virtual"].y = torch.from_numpy(rng.integers(0, NUM_ROOM_LABELS, size=n_rooms).astype(np.int64))
    for k, et in enumerate(HTREE_INIT_EDGE_TYPES):
        key = f"g{gi}_i{k}"
        if key in npz:
            g[et].edge_index = torch.from_numpy(npz[key].astype(np.int64).reshape(2, -1))
    return g


def htree_batch(batch_size: int = 128, seed: int = BASE_SEED + 4, fixture: Optional[str] = None) -> HeteroData:
    """Config 4 (``seed = BASE_SEED + 4``): the fixture's topologies tiled to ``batch_size`` graphs, fresh features/labels."""
    npz = np.load(fixture or HTREE_FIXTURE)
    rng = np.random.Generator(np.random.PCG64(seed))
    n = int(npz["n_graphs"])
    return collate([htree_graph(npz, i % n, rng) for i in range(batch_size)])


def semisupervised_htree_batch(n_graphs: int, seed: int, relative_pos: bool = False) -> HeteroData:
    """Batch of the two-headed task on H-trees (``HeterogeneousNeuralTreeNetwork(output_dim_dict=...)``,
    ``SemiSupervisedTrainingJob`` on Stanford3DSG): the committed fixture's topologies as in ``htree_batch``, ``room_virtual.y`` in
    0..14 and ``object_virtual.y`` in 0..34, and a seeded per-node split of BOTH virtual types into disjoint ``train_mask`` (60 %),
    ``val_mask`` (20 %) and ``test_mask`` (20 %).  ``relative_pos``: 3-d ``edge_attr`` (destination minus source xyz, the leading
    columns of ``x``) on the message-passing edge types, for GAT_edge; the pool edges carry none."""
    npz = np.load(HTREE_FIXTURE)
    rng = np.random.Generator(np.random.PCG64(seed))
    n = int(npz["n_graphs"])
    graphs = [htree_graph(npz, i % n, rng) for i in range(n_graphs)]
    for g in graphs:
        for t, classes in (("room_virtual", 15), ("object_virtual", 35)):
            g[t].y = torch.from_numpy(rng.integers(0, classes, size=int(g[t].num_nodes)).astype(np.int64))
        if relative_pos:
            for src, rel, dst in HTREE_EDGE_TYPES:
                ei = g[src, rel, dst].edge_index
                g[src, rel, dst].edge_attr = (g[dst].x[ei[1], :3] - g[src].x[ei[0], :3]).contiguous()
    batch = collate(graphs)
    for t in ("room_virtual", "object_virtual"):
        u = torch.from_numpy(rng.random(int(batch[t].y.numel())))
        batch[t].train_mask = u < 0.6
        batch[t].val_mask = (u >= 0.6) & (u < 0.8)
        batch[t].test_mask = u >= 0.8
    return batch


# ---------------------------------------------------------------------------------------------------------------------
# config 2, second input: the reference's real scene graph replicated x B
# ---------------------------------------------------------------------------------------------------------------------
DSG_FIXTURE = os.path.join(os.path.dirname(HTREE_FIXTURE), "dsg_x8F5xyUWy9e.json")


def real_fixture_frame(fixture: Optional[str] = None, seed: int = BASE_SEED) -> HeteroData:
    """The reference's test scene graph (``tests/test_data/x8F5xyUWy9e_0_gt_partial_dsg_1447.json``, static layers committed as
    ``tests/golden/dsg_x8F5xyUWy9e.json``) through the engine's own reader with the training thresholds
    (``prepare_hydra_mp3d_training.py:24-26``): 5 rooms, 62 objects, 356 + 2 + 62 + 62 directed edges.  The 300-d semantic block
    is a seeded per-label table (word2vec is a download); room labels are drawn (the bench needs a loss, not these labels).
    Object connectivity runs on the device (``csrc/dsg.hip``): needs the GPU."""
    from . import dsg

    rog = dsg.RoomObjectGraph(dsg.load_dsg_json(fixture or DSG_FIXTURE))
    rng = np.random.Generator(np.random.PCG64(seed))
    table = rng.normal(0.0, 0.15, size=(int(rog.sg.label[rog.objects].max()) + 1, 300))
    oo = dsg.object_connectivity(rog, 1.5, 2.0, 0.2)
    frame = dsg.to_hetero_data(rog, oo, {"objects": table[rog.sg.label[rog.objects]]}).to("cpu")
    frame["rooms"].y = torch.from_numpy(rng.integers(0, NUM_ROOM_LABELS, size=len(rog.rooms)))
    return frame


def real_fixture_batch(batch_size: int = 32, fixture: Optional[str] = None) -> HeteroData:
    return collate([real_fixture_frame(fixture)] * batch_size)


# ---------------------------------------------------------------------------------------------------------------------
# two-headed task, per-graph form: what SemiSupervisedTrainingJob's DataLoader iterates over (a dataset is a LIST of graphs,
# each carrying its own train / val / test split) and what store.GraphStore keeps on the device.  Four data shapes.
# ---------------------------------------------------------------------------------------------------------------------
def _split_masks(rng: np.random.Generator, n: int):
    """seeded disjoint 60 / 20 / 20 split of n rows: (train_mask, val_mask, test_mask) bool tensors"""
    u = torch.from_numpy(rng.random(n))
    return u < 0.6, (u >= 0.6) & (u < 0.8), u >= 0.8


def semisupervised_graphs(n_graphs: int, seed: int, relative_pos: bool = False) -> List[HeteroData]:
    """``mp3d_like_graph`` graphs of the two-headed task (``HeterogeneousNetwork(output_dim_dict=...)``): room labels 0..25, object
    labels 0..27, ``train_mask`` / ``val_mask`` / ``test_mask`` on BOTH node types of every graph."""
    rng = np.random.Generator(np.random.PCG64(seed))
    graphs = [mp3d_like_graph(rng) for _ in range(n_graphs)]
    for g in graphs:
        if relative_pos:
            compute_relative_pos(g)
        for t in ("rooms", "objects"):
            g[t].train_mask, g[t].val_mask, g[t].test_mask = _split_masks(rng, int(g[t].y.numel()))
    return graphs


def semisupervised_htree_graphs(n_graphs: int, seed: int, relative_pos: bool = False) -> List[HeteroData]:
    """H-tree graphs of the two-headed task (``HeterogeneousNeuralTreeNetwork(output_dim_dict=...)``), per graph what
    ``semisupervised_htree_batch`` is per batch: the committed fixture's topologies, ``room_virtual.y`` in 0..14,
    ``object_virtual.y`` in 0..34, the three masks on both virtual types; ``relative_pos``: 3-d ``edge_attr`` on the
    message-passing edge types."""
    npz = np.load(HTREE_FIXTURE)
    rng = np.random.Generator(np.random.PCG64(seed))
    n = int(npz["n_graphs"])
    graphs = [htree_graph(npz, i % n, rng) for i in range(n_graphs)]
    for g in graphs:
        for t, classes in (("room_virtual", 15), ("object_virtual", 35)):
            g[t].y = torch.from_numpy(rng.integers(0, classes, size=int(g[t].num_nodes)).astype(np.int64))
            g[t].train_mask, g[t].val_mask, g[t].test_mask = _split_masks(rng, int(g[t].num_nodes))
        if relative_pos:
            for src, rel, dst in HTREE_EDGE_TYPES:
                ei = g[src, rel, dst].edge_index
                g[src, rel, dst].edge_attr = (g[dst].x[ei[1], :3] - g[src].x[ei[0], :3]).contiguous()
    return graphs


def stanford_semisupervised_graphs(n_graphs: int, seed: int, edge_attr: bool = False) -> List[Data]:
    """``stanford_like_graph``s of the homogeneous two-headed task (``HomogeneousNetwork(output_dim_dict=...)``): ``x``, ``y``,
    ``edge_index``, ``room_mask`` and the three masks per graph; ``edge_attr``: 3-d relative positions for GAT_edge."""
    rng = np.random.Generator(np.random.PCG64(seed))
    graphs = [stanford_like_graph(rng) for _ in range(n_graphs)]
    for g in graphs:
        g.train_mask, g.val_mask, g.test_mask = _split_masks(rng, g.num_nodes)
        if edge_attr:
            g.edge_attr = (g.x[g.edge_index[1], :3] - g.x[g.edge_index[0], :3]).contiguous()
    return graphs


def stanford_htree_semisupervised_graphs(n_graphs: int, seed: int, edge_attr: bool = False) -> List[Data]:
    """Homogeneous H-tree graphs of the two-headed task (``HomogeneousNeuralTreeNetwork(output_dim_dict=...)``): the fixture's
    H-trees through ``heterogeneous_htree_to_homogeneous`` with 6-d features -- ``x``, ``y`` (rooms 0..14 on the ``room_mask`` rows,
    objects 0..34 elsewhere), ``edge_index`` / ``init_edge_index`` / ``pool_edge_index``, ``node_type``, ``room_mask``,
    ``object_mask`` and the three masks per graph."""
    from .data import heterogeneous_htree_to_homogeneous

    npz = np.load(HTREE_FIXTURE)
    rng = np.random.Generator(np.random.PCG64(seed))
    n = int(npz["n_graphs"])
    graphs = []
    for i in range(n_graphs):
        d = heterogeneous_htree_to_homogeneous(htree_graph(npz, i % n, rng))
        del d.__dict__["edge_type"]
        d.x = d.x[:, :6].contiguous()
        N = d.num_nodes
        y = torch.from_numpy(rng.integers(0, 35, size=N).astype(np.int64))
        y[d.room_mask] = torch.from_numpy(rng.integers(0, 15, size=int(d.room_mask.sum())).astype(np.int64))
        d.y = y
        d.train_mask, d.val_mask, d.test_mask = _split_masks(rng, N)
        if edge_attr:
            d.edge_attr = (d.x[d.edge_index[1], :3] - d.x[d.edge_index[0], :3]).contiguous()
        graphs.append(d)
    return graphs


def synthetic_scene(n_objects: int, n_rooms: int, seed: int = 0, n_labels: int = 41, places_per_room: int = 4):
    """Static layers of a synthetic scene graph as the flat arrays ``dsg.FramePipeline.convert`` reads:
    ``(ids, layer, pos, bb_min, bb_max, label, edges)``.  One building, ``n_rooms`` rooms in a chain, ``places_per_room`` places
    per room in a chain, ``n_objects`` objects spread over the places; node ids are spark_dsg NodeSymbols (category letter in the
    top byte), the arrays are in shuffled order (layers are visited in ascending id, not in array order)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sym = lambda c, i: (ord(c) << 56) + i
    ids, layer, pos, half, label, edges = [], [], [], [], [], []

    def node(i, lay, p, h, lab):
        ids.append(i), layer.append(lay), pos.append(p), half.append(h), label.append(lab)
        return i

    b = node(sym("B", 0), 5, np.zeros(3), np.ones(3), 0)
    places = []
    for r in range(n_rooms):
        centre = np.array([8.0 * r, 0.0, 1.5])
        room = node(sym("R", r), 4, centre, np.ones(3), int(rng.integers(0, 25)))
        edges.append((b, room))
        if r:
            edges.append((sym("R", r - 1), room))
        for k in range(places_per_room):
            p = node(sym("p", r * places_per_room + k), 3, centre + rng.normal(0, 1.5, 3), 0.5 * np.ones(3), 0)
            edges.append((room, p))
            if k:
                edges.append((sym("p", r * places_per_room + k - 1), p))
            places.append(p)
    index = {v: i for i, v in enumerate(ids)}
    for o in range(n_objects):
        p = places[int(rng.integers(0, len(places)))]
        obj = node(sym("O", o), 2, pos[index[p]] + rng.normal(0, 1.2, 3), rng.uniform(0.1, 0.8, 3), int(rng.integers(0, n_labels)))
        edges.append((obj, p))
    perm = rng.permutation(len(ids))
    ids = np.array(ids, dtype=np.uint64)[perm]
    pos, half = np.array(pos, dtype=np.float64)[perm], np.array(half, dtype=np.float64)[perm]
    return (ids, np.array(layer, dtype=np.int32)[perm], pos, pos - half, pos + half, np.array(label, dtype=np.int64)[perm],
            np.array(edges, dtype=np.uint64).reshape(-1, 2).T.copy())
