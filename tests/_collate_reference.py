"""Numpy reference of batch collation (csrc/collate.hip) and the builders of its test cases.

A packed dataset is what ``GraphStore`` keeps on the device: per *slot* (a node type or an edge type) a ``[G + 1]`` offset vector,
and per *item* one array positioned by a slot: rows of ``row_bytes`` bytes (features, labels, masks, edge attributes) or an int64
``[2][E]`` edge list with graph-local indices.  A batch is the graphs ``sel[0 .. B)``, repeats allowed:

  rows    the rows of the selected graphs back to back, in selection order                       (byte moves)
  edges   the edge lists back to back, each endpoint shifted by the number of nodes the graphs in front of it in the
          selection have in that endpoint's slot                                                  (integer adds)

so the reference is exact.  Plain loops over the graphs of the selection; nothing here touches the device or the library.
tests/test_collate_reference.py holds it against ``hydra_gnn_amd.data.collate``."""
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np


def collate_rows_ref(src: np.ndarray, ptr: np.ndarray, sel: Sequence[int]) -> np.ndarray:
    """``src``: ``uint8 [rows][row_bytes]`` (any dtype and width, viewed as bytes); returns ``uint8 [n_out][row_bytes]``"""
    assert src.dtype == np.uint8 and src.ndim == 2
    out = np.empty((0, src.shape[1]), np.uint8)
    for g in sel:
        out = np.concatenate([out, src[int(ptr[g]):int(ptr[g + 1])]], axis=0)
    return out


def collate_edges_ref(ei: np.ndarray, edge_ptr: np.ndarray, sel: Sequence[int], node_ptr_src: np.ndarray,
                      node_ptr_dst: np.ndarray) -> np.ndarray:
    """``ei``: ``int64 [2][E]`` with graph-local indices; returns ``int64 [2][e_out]``.  The shifts are the cumulative node counts of
    the selection (a graph selected twice counts twice), not the dataset's offsets."""
    assert ei.dtype == np.int64 and ei.ndim == 2 and ei.shape[0] == 2
    out = np.empty((2, 0), np.int64)
    n_src = n_dst = 0
    for g in sel:
        part = ei[:, int(edge_ptr[g]):int(edge_ptr[g + 1])] + np.array([[n_src], [n_dst]], np.int64)
        out = np.concatenate([out, part], axis=1)
        n_src += int(node_ptr_src[g + 1] - node_ptr_src[g])
        n_dst += int(node_ptr_dst[g + 1] - node_ptr_dst[g])
    return out


def offsets_ref(ptrs: Sequence[np.ndarray], sel: Sequence[int]):
    """the ``[n_slots][B + 1]`` table (``Batch.ptr`` of every slot) and the ``[n_slots]`` totals"""
    table = np.zeros((len(ptrs), len(sel) + 1), np.int64)
    for s, p in enumerate(ptrs):
        for b, g in enumerate(sel):
            table[s, b + 1] = table[s, b] + int(p[g + 1] - p[g])
    return table, table[:, -1].copy()


# ---------------------------------------------------------------------------------------------------------------------------
# case builders
# ---------------------------------------------------------------------------------------------------------------------------
@dataclass
class RowItem:
    slot: int
    row_bytes: int
    data: Optional[np.ndarray]  # uint8 [rows][row_bytes]; None: no source array (a slot that is empty in every graph)


@dataclass
class EdgeItem:
    slot: int
    slot_src: int
    slot_dst: int
    ei: Optional[np.ndarray]  # int64 [2][E]


@dataclass
class Dataset:
    n_graphs: int
    ptrs: List[np.ndarray]
    items: list = field(default_factory=list)

    def counts(self, slot):
        return np.diff(self.ptrs[slot])

    def expected(self, sel):
        """per item the collated array as bytes (rows: ``uint8 [n_out * row_bytes]``; edges: the ``[2][e_out]`` list as bytes)"""
        out = []
        for it in self.items:
            if isinstance(it, RowItem):
                src = it.data if it.data is not None else np.empty((0, it.row_bytes), np.uint8)
                out.append(collate_rows_ref(src, self.ptrs[it.slot], sel).reshape(-1))
            else:
                ei = it.ei if it.ei is not None else np.empty((2, 0), np.int64)
                e = collate_edges_ref(ei, self.ptrs[it.slot], sel, self.ptrs[it.slot_src], self.ptrs[it.slot_dst])
                out.append(np.ascontiguousarray(e).view(np.uint8).reshape(-1))
        return out


#: graphs every ragged count vector leaves empty: the first, the last and a run of three in the middle (G >= 9)
def forced_empty(n_graphs):
    assert n_graphs >= 9
    m = n_graphs // 2
    return [0, m - 1, m, m + 1, n_graphs - 1]


def ragged_counts(rng, n_graphs, hi, zero_share=0.25):
    """per-graph counts in ``[1, hi]`` with ``zero_share`` of them (and the ``forced_empty`` graphs) zero"""
    c = rng.integers(1, hi + 1, size=n_graphs)
    c[rng.random(n_graphs) < zero_share] = 0
    c[forced_empty(n_graphs)] = 0
    return c.astype(np.int64)


def ptr_of(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def random_rows(rng, n_rows, row_bytes):
    return rng.integers(0, 256, size=(int(n_rows), int(row_bytes)), dtype=np.uint8)


def random_edges(rng, edge_counts, src_counts, dst_counts):
    """graph-local endpoints below the graph's node counts; a graph without nodes at either end gets no edge"""
    edge_counts = np.where((src_counts > 0) & (dst_counts > 0), edge_counts, 0).astype(np.int64)
    parts = [np.stack([rng.integers(0, src_counts[g], size=e), rng.integers(0, dst_counts[g], size=e)]) if e else np.empty((2, 0), np.int64)
             for g, e in enumerate(edge_counts)]
    return edge_counts, np.ascontiguousarray(np.concatenate(parts, axis=1), dtype=np.int64)


def make_dataset(seed, n_graphs, slot_hi, row_items, edge_items=(), zero_share=0.25, empty_slots=()):
    """``slot_hi[s]``: the largest per-graph count of node slot ``s``; ``row_items``: ``(slot, row_bytes)``; ``edge_items``:
    ``(slot_src, slot_dst, hi)``, each an edge slot of its own behind the node slots and the item of its edge list; row items may be
    positioned by an edge slot (edge attributes).  ``empty_slots``: node slots without a row in any graph."""
    rng = np.random.default_rng(seed)
    counts = [np.zeros(n_graphs, np.int64) if s in empty_slots else ragged_counts(rng, n_graphs, hi, zero_share)
              for s, hi in enumerate(slot_hi)]
    edges = []
    for ss, sd, hi in edge_items:
        # besides the graphs without a node at one end: the forced ones and one graph that has nodes at both ends
        ec = ragged_counts(rng, n_graphs, hi, 0.0)
        ec[rng.choice(np.flatnonzero((counts[ss] > 0) & (counts[sd] > 0)))] = 0
        ec, ei = random_edges(rng, ec, counts[ss], counts[sd])
        assert (ec > 0).sum() >= 3, "too few graphs with nodes at both ends: more graphs or a smaller zero_share"
        edges.append(EdgeItem(len(counts), ss, sd, ei))
        counts.append(ec)
    ds = Dataset(n_graphs, [ptr_of(c) for c in counts])
    for slot, rb in row_items:
        ds.items.append(RowItem(slot, rb, random_rows(rng, ds.ptrs[slot][-1], rb)))
    ds.items.extend(edges)
    return ds


def ragged_selections(ds, slot, seed):
    """the selections of the issue for ``slot``: one graph; five with repeats; one that starts, ends and has a middle run of graphs
    empty in ``slot``; only graphs that are empty in ``slot``"""
    rng = np.random.default_rng(seed)
    c = ds.counts(slot)
    full, empty = np.flatnonzero(c > 0), np.flatnonzero(c == 0)
    forced = forced_empty(ds.n_graphs)  # empty in every slot: the others first, so that the other slots have rows
    empty = np.array([g for g in empty if g not in forced] + [g for g in empty if g in forced])
    assert len(full) >= 3 and len(empty) >= 3
    a, b, d = (int(x) for x in full[:3])
    e0, e1, e2 = (int(x) for x in empty[:3])
    return {
        "one": [int(full[-1])],
        "repeats": [a, b, a, int(rng.choice(ds.n_graphs)), b],
        "empty_edges_and_run": [e0, e1, a, b, e2, e0, e1, d, a, e2, e2],
        "only_empty": [e0, e2, e1, e0],
    }
