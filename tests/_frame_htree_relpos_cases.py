"""Shared cases of the tests of relative positions on H-tree edges (``FramePipeline(htree=True, htree_relative_pos=True)``;
tests/test_frame_htree_relpos_host.py, tests/test_gpu_frame_htree_relpos.py): the frames, the Python oracle
(``data.compute_relative_pos`` of ``htree.generate_htree(..., clique_pos=True)``) and the tolerance rule.  The numpy execution of a
packed block, the item kind the mode adds (``HMP_FK_EATTR_HT``) included, is tests/_frame_block.py."""
import numpy as np
import torch

import _frame_batch_cases as bc
import _frame_cases as fc
from hydra_gnn_amd import _lib, data as hdata, dsg, htree, workloads

CLIQUE_DIM = 6
EDGE_KEYS = [k for k, a in dsg._FRAME_TENSORS[_lib.FT_HTREE:] if a == "edge_index"]  # 10 tree, 3 init, o_to_ov, r_to_rv
POOL_KEYS = EDGE_KEYS[13:]
CLIQUE_TYPES = {"object-room": 2, "room-room": 3}
_CACHE = {}


def frame(name):
    """``fc.frame`` plus "triangle": four rooms 0-1-2-3 in a chain with the chords 0-2 and 1-3, so that the room-room cliques
    {0, 1, 2} and {1, 2, 3} have three members each (and an rr_to_rr edge joins them)"""
    if name != "triangle":
        return bc.frame(name)
    if name not in _CACHE:
        ids, layer, pos, bb_min, bb_max, label, edges = workloads.synthetic_scene(9, 4, seed=23)
        sym = lambda c, i: (ord(c) << 56) + i
        more = np.array([[sym("R", 0), sym("R", 1)], [sym("R", 2), sym("R", 3)]], dtype=np.uint64)
        _CACHE[name] = (ids, layer, pos, bb_min, bb_max, label, np.concatenate([np.asarray(edges, dtype=np.uint64), more], axis=1))
    return _CACHE[name]


# one room (no room-room clique, zero-row tensors): (1, 1), (65, 1); a clique of three rooms: "triangle"; tree edge types without an
# edge: every case but "triangle" has some
CASES = ["fixture", "special", "triangle"] + fc.SIZES
SMALL_CASES = ["fixture", "special", "triangle", (1, 1), (7, 2), (65, 1)]


def host_kwargs(homogeneous, sem=False):
    tn, mn, mo = fc.THRESHOLDS
    return dict(threshold_near=tn, max_near=mn, max_on=mo, htree=True, htree_relative_pos=True, sem_dim=300 if sem else 0,
                n_labels=fc.N_LABELS if sem else 0, clique_dim=CLIQUE_DIM, homogeneous=homogeneous)


def pipeline_kwargs(homogeneous, sem=False):
    return dict(semantic_table=fc.semantic_table() if sem else None, htree=True, htree_relative_pos=True, clique_dim=CLIQUE_DIM,
                homogeneous=homogeneous)


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
def oracle_typed(arrays, sem=False, device="cpu"):
    """``compute_relative_pos(generate_htree(frame, CLIQUE_DIM, clique_pos=True))`` of the existing path; also returns the tree
    BEFORE the three columns were dropped (its clique members and room positions give the tolerance)"""
    g, _ = fc.existing_frame(arrays, sem, device=device)
    tree = htree.generate_htree(g, clique_dim=CLIQUE_DIM, clique_pos=True)
    members = {t: fc.clique_members(tree, k) for t, k in CLIQUE_TYPES.items()}
    rpos = tree["room_virtual"].pos.cpu().numpy()
    hdata.compute_relative_pos(tree)
    return tree, members, rpos


def clique_bound(members, rpos):
    """per clique: 0 for up to two member rooms (two float32 additions from zero and a division by 1 or 2 have one result in any
    order), else k * 2^-24 * max|coordinate| over its k members -- the bound DESIGN 6.9 states for clique means"""
    return np.array([0.0 if len(m) <= 2 else len(m) * 2.0 ** -24 * float(np.abs(rpos[m]).max()) for m in members], dtype=np.float64)


def assert_close_rows(got, want, bound, what):
    """rows with bound 0 bit for bit, the others within their bound"""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    exact = bound == 0
    assert np.array_equal(got[exact], want[exact]), what
    if (~exact).any():
        assert (np.abs(got[~exact].astype(np.float64) - want[~exact]) <= bound[~exact, None]).all(), what


def edge_bound(key, ei, bounds):
    """per edge: the sum of the bounds of its clique ends"""
    b = np.zeros(ei.shape[1], dtype=np.float64)
    for row, t in ((0, key[0]), (1, key[2])):
        if t in bounds:
            b += bounds[t][ei[row]]
    return b


def typed_graph(views):
    """a ``HeteroData`` from {(key, attr): numpy array} (copies), stores in the pipeline's order"""
    g = hdata.HeteroData()
    for t in dsg._HTREE_STORES:
        g[t]
    for (key, attr), a in views.items():
        setattr(g[key], attr, torch.from_numpy(np.array(a)))
    return g
