"""Shared cases of the derived-store tests (tests/test_store_derive_host.py, tests/test_gpu_store_derive.py,
tests/test_gpu_store_node_split.py, tests/test_gpu_store_dataset_jobs.py): small typed graphs that cover the corner cases, small
H-trees, the host transforms a derived store is compared against, and the store comparison."""
import numpy as np
import torch

from hydra_gnn_amd import data as hdata, htree
from hydra_gnn_amd.data import Data, HeteroData
from hydra_gnn_amd.store import _Packed

OO = ("objects", "objects_to_objects", "objects")
RR = ("rooms", "rooms_to_rooms", "rooms")
OR = ("objects", "objects_to_rooms", "rooms")
RO = ("rooms", "rooms_to_objects", "objects")
# (objects, rooms): one graph with a single room, one with a single object
BASELINE_COUNTS = [(5, 2), (3, 1), (1, 3), (7, 2), (4, 4)]
OBJ_W, ROOM_W = 9, 6  # objects wider than rooms: the homogeneous x is padded


def _edges(rng, n_src, n_dst, n):
    return torch.from_numpy(np.stack([rng.integers(0, n_src, n), rng.integers(0, n_dst, n)]).astype(np.int64))


def baseline_graphs(with_y=True, obj_w=OBJ_W, room_w=ROOM_W, counts=BASELINE_COUNTS, seed=5, ro_edges=False):
    """Typed baseline graphs: ``x`` starts with the position columns; ``rooms_to_rooms`` is empty in the single-room graph and
    ``rooms_to_objects`` in every graph (``ro_edges``: the flipped ``objects_to_rooms`` instead -- a stream cannot collate an edge type
    that is empty in the whole store); ``y`` on both node types or on none."""
    rng = np.random.default_rng(seed)
    out = []
    for gi, (n_o, n_r) in enumerate(counts):
        g = HeteroData()
        for t, n, w in (("objects", n_o, obj_w), ("rooms", n_r, room_w)):
            x = torch.from_numpy(rng.standard_normal((n, w)).astype(np.float32))
            g[t].x = x
            g[t].pos = x[:, :3].clone()
            if with_y:
                g[t].y = torch.from_numpy(rng.integers(0, 15, n).astype(np.int64))
        g[OO].edge_index = _edges(rng, n_o, n_o, 2 * n_o + gi)
        g[RR].edge_index = _edges(rng, n_r, n_r, 0 if n_r == 1 else n_r + 1)
        g[OR].edge_index = _edges(rng, n_o, n_r, n_o)
        g[RO].edge_index = g[OR].edge_index.flip(0) if ro_edges else torch.empty((2, 0), dtype=torch.int64)
        out.append(g)
    return out


def htree_graphs(with_y=True, n=4, seed=9):
    """small H-trees with a ``pos`` on every node type (``clique_pos=True``): object_virtual / room_virtual carry ``y``, the leaves
    their copies, the clique types none"""
    base = baseline_graphs(with_y, counts=[(4, 2), (3, 1), (6, 3), (2, 2), (5, 2), (1, 1)][:n], seed=seed)
    for g in base:  # a connected room layer and every object in a room: what the H-tree is built from
        n_o, n_r = g["objects"].num_nodes, g["rooms"].num_nodes
        chain = torch.arange(n_r - 1, dtype=torch.int64)
        g[RR].edge_index = torch.stack([chain, chain + 1]) if n_r > 1 else torch.empty((2, 0), dtype=torch.int64)
        g[RO].edge_index = torch.stack([torch.arange(n_o, dtype=torch.int64) % n_r, torch.arange(n_o, dtype=torch.int64)])
        g[OR].edge_index = g[RO].edge_index.flip(0)
    return [htree.generate_htree(g, clique_dim=ROOM_W, clique_pos=True) for g in base]


def clone(g):
    """a graph with its own containers and tensors"""
    if not hasattr(g, "node_types"):
        return Data(**{k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in g.__dict__.items() if k != "_plan_cache"})
    out = HeteroData()
    for key in g.node_types + g.edge_types:
        for k, v in g[key].items():
            if k not in ("ptr", "ptr_version"):
                setattr(out[key], k, v.clone() if isinstance(v, torch.Tensor) else v)
    return out


# ---- the host transforms (what the reference's scripts apply to a loaded dataset, graph by graph) --------------------------------
def relative_pos(g):
    hdata.compute_relative_pos(g)
    return g


def homogeneous(g):
    if "object_virtual" in g.node_types:
        return hdata.heterogeneous_htree_to_homogeneous(g)
    d, types = hdata.heterogeneous_data_to_homogeneous(g)
    d.room_mask = d.node_type == types.index("rooms")
    return d


def remove_last_features(g, dim):
    """reference mp3d_dataset.py:286-296"""
    if hasattr(g, "node_types"):
        for t in g.x_dict:
            if g[t].num_node_features >= dim:
                g[t].x = g[t].x[:, :-dim]
    elif g.x.size(1) >= dim:
        g.x = g.x[:, :-dim]
    return g


# ---- comparison --------------------------------------------------------------------------------------------------------------------
SKIP = ("lib", "_stage", "_stage_dev", "_copied", "_split")


def assert_same_value(g, w, what):
    if isinstance(w, _Packed):
        assert isinstance(g, _Packed), what
        return assert_same_value(vars(g), vars(w), what)
    if isinstance(w, dict):
        assert list(g) == list(w), (what, list(g), list(w))  # same keys in the same order: collate walks them
        for k in w:
            assert_same_value(g[k], w[k], (what, k))
    elif isinstance(w, torch.Tensor):
        assert g.dtype == w.dtype and g.shape == w.shape and g.device == w.device and g.is_contiguous(), (what, g.dtype, g.shape, w.dtype, w.shape)
        assert torch.equal(g, w), what
        if w.dtype == torch.bool:  # a byte that was never written is "true" too: compare the bytes
            assert torch.equal(g.view(torch.uint8), w.view(torch.uint8)), what
    elif isinstance(w, np.ndarray):
        assert g.dtype == w.dtype and np.array_equal(g, w), what
    else:
        assert g == w, (what, g, w)


def assert_same_store(got, want):
    """every packed array, every device and host offset vector, node_types, edge_types, homo_keys, edge_name, edge_rows, count_only"""
    assert sorted(k for k in vars(got) if k not in SKIP) == sorted(k for k in vars(want) if k not in SKIP)
    for k, w in vars(want).items():
        if k not in SKIP:
            assert_same_value(getattr(got, k), w, k)
