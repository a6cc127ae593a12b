"""The numpy collation reference of tests/_collate_reference.py equals ``hydra_gnn_amd.data.collate`` (PyG's rule) on small hetero
graphs built on the spot: node rows, int64 labels, a bool mask, the edge lists of a same-type and a two-type edge, ``edge_attr``;
repeated ids, graphs without a node of one type and graphs without an edge of one type.  Needs no GPU."""
import numpy as np
import pytest
import torch

import _collate_reference as R
from hydra_gnn_amd.data import HeteroData, collate

AA, AB = ("a", "aa", "a"), ("a", "ab", "b")
N_A = [4, 1, 6, 3, 2, 5]
N_B = [2, 3, 0, 1, 0, 4]      # graphs 2 and 4 have no `b` node, hence no a->b edge
E_AA = [5, 0, 9, 0, 1, 7]     # graphs 1 and 3 have no a->a edge
E_AB = [3, 2, 0, 4, 0, 0]     # graph 5 has `b` nodes but no a->b edge


def graphs():
    rng = np.random.default_rng(11)
    gs = []
    for na, nb, eaa, eab in zip(N_A, N_B, E_AA, E_AB):
        g = HeteroData()
        g["a"].x = torch.from_numpy(rng.standard_normal((na, 5)).astype(np.float32))
        g["a"].y = torch.from_numpy(rng.integers(0, 26, size=na))
        g["a"].mask = torch.from_numpy(rng.random(na) < 0.5)
        g["b"].x = torch.from_numpy(rng.standard_normal((nb, 2)).astype(np.float32))
        g[AA].edge_index = torch.from_numpy(rng.integers(0, na, size=(2, eaa)))
        g[AB].edge_index = torch.from_numpy(np.stack([rng.integers(0, na, size=eab), rng.integers(0, max(nb, 1), size=eab)]))
        g[AA].edge_attr = torch.from_numpy(rng.standard_normal((eaa, 3)).astype(np.float32))
        g[AB].edge_attr = torch.from_numpy(rng.standard_normal((eab, 3)).astype(np.float32))
        gs.append(g)
    return gs


def as_bytes(t):
    """[rows, ...] tensor -> uint8 [rows][row_bytes]"""
    a = np.ascontiguousarray(t.numpy())
    return a.view(np.uint8).reshape(a.shape[0], int(np.prod(a.shape[1:])) * a.itemsize)


def pack(gs, get):
    """packed array of one attribute over all graphs + its [G + 1] offsets, as GraphStore keeps them"""
    parts = [get(g) for g in gs]
    return torch.cat(parts, dim=0), R.ptr_of([p.size(0) for p in parts])


@pytest.fixture(scope="module")
def packed():
    gs = graphs()
    ptr = {"a": R.ptr_of(N_A), "b": R.ptr_of(N_B), AA: R.ptr_of(E_AA), AB: R.ptr_of(E_AB)}
    return gs, ptr


@pytest.mark.parametrize("ids", [[0], [3, 1, 4, 1, 5], [2, 2, 2], [4, 2], [5, 0, 3, 3, 1, 2, 4, 0]])
def test_reference_equals_host_collate(packed, ids):
    gs, ptr = packed
    ref = collate([gs[i] for i in ids])
    for t, k in (("a", "x"), ("a", "y"), ("a", "mask"), ("b", "x")):
        src, p = pack(gs, lambda g: getattr(g[t], k))
        assert np.array_equal(p, ptr[t])
        want = getattr(ref[t], k)
        got = R.collate_rows_ref(as_bytes(src), ptr[t], ids)
        assert got.dtype == np.uint8 and got.shape == (want.size(0), src[0].numel() * src.element_size())
        assert np.array_equal(got, as_bytes(want)), (t, k)
    for e in (AA, AB):
        ei = np.ascontiguousarray(torch.cat([g[e].edge_index for g in gs], dim=1).numpy())
        got = R.collate_edges_ref(ei, ptr[e], ids, ptr[e[0]], ptr[e[2]])
        assert got.dtype == np.int64 and np.array_equal(got, ref[e].edge_index.numpy()), e
        src, p = pack(gs, lambda g: g[e].edge_attr)
        assert np.array_equal(p, ptr[e])
        assert np.array_equal(R.collate_rows_ref(as_bytes(src), ptr[e], ids), as_bytes(ref[e].edge_attr)), e
    keys = ["a", "b", AA, AB]
    table, totals = R.offsets_ref([ptr[k] for k in keys], ids)
    assert table.shape == (4, len(ids) + 1) and table.dtype == np.int64
    for s, k in enumerate(keys):
        assert np.array_equal(table[s], ref[k].ptr.numpy()), k
    assert totals.tolist() == [ref["a"].x.size(0), ref["b"].x.size(0), ref[AA].edge_index.size(1), ref[AB].edge_index.size(1)]


def test_dataset_expected_goes_through_the_same_functions(packed):
    """Dataset.expected (what the GPU tests compare with) is the three functions above applied item by item"""
    gs, ptr = packed
    x, _ = pack(gs, lambda g: g["a"].x)
    m, _ = pack(gs, lambda g: g["a"].mask)
    ei = np.ascontiguousarray(torch.cat([g[AB].edge_index for g in gs], dim=1).numpy())
    ds = R.Dataset(len(gs), [ptr["a"], ptr["b"], ptr[AB]],
                   [R.RowItem(0, 20, as_bytes(x)), R.RowItem(0, 1, as_bytes(m)), R.EdgeItem(2, 0, 1, ei)])
    ids = [3, 1, 4, 1, 5]
    ref = collate([gs[i] for i in ids])
    got = ds.expected(ids)
    assert np.array_equal(got[0], as_bytes(ref["a"].x).reshape(-1))
    assert np.array_equal(got[1], as_bytes(ref["a"].mask).reshape(-1))
    assert np.array_equal(got[2].view(np.int64).reshape(2, -1), ref[AB].edge_index.numpy())


def test_builders_make_the_ragged_shapes_the_gpu_cases_rely_on():
    ds = R.make_dataset(3, 24, [7, 5], [(0, 12), (1, 3), (2, 12)], edge_items=[(0, 1, 6)])
    for s in range(3):
        c = ds.counts(s)
        assert c[0] == 0 and c[-1] == 0 and (c[11:14] == 0).all() and (c > 0).sum() >= 3
    c = [ds.counts(s) for s in range(3)]
    assert ((c[2] == 0) & (c[0] > 0) & (c[1] > 0)).sum() >= 1  # a graph with nodes at both ends and no edge
    e = ds.items[-1]
    for g in range(24):  # graph-local endpoints
        part = e.ei[:, ds.ptrs[2][g]:ds.ptrs[2][g + 1]]
        assert part.shape[1] == 0 or (part[0].max() < ds.counts(0)[g] and part[1].max() < ds.counts(1)[g] and part.min() >= 0)
    sels = R.ragged_selections(ds, 0, 1)
    c = ds.counts(0)
    assert len(sels["one"]) == 1 and len(sels["repeats"]) == 5 and len(set(sels["repeats"])) < 5
    s = sels["empty_edges_and_run"]
    assert c[s[0]] == 0 and c[s[1]] == 0 and c[s[-1]] == 0 and c[s[-2]] == 0 and (c[s[4:7]] == 0).all() and c[s].sum() > 0
    assert c[sels["only_empty"]].sum() == 0
