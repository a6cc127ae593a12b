"""Host-side helpers of the SAGE aggregation tests (no GPU; the leading underscore keeps pytest from collecting it).

* A plain-Python mirror of the launch decisions of the SAGE aggregation (csrc/aggregate.hip, csrc/net.hip): which kernel
  instantiation a network of a given shape launches per layer and direction, whether the cross entropy rides in the last
  aggregation and at which row-group width, 8-row tiles, the XCD row mapping, LDS-window eligibility and the ids a window
  chunk stages.  tests/test_sage_dispatch.py checks that the GPU cases reach every instantiation through it.
* sage_regime_scene: an mp3d-schema scene whose every edge type carries the in-degree classes at which the batching of
  agg_row / agg_bwd_row changes (0, 1, 7..9, 15..17, 24, 31..33, 64, 65, a hub) in both directions, and check_sage_regimes.
* window_graph: a config-5-shaped graph with window chunks over the LDS id capacity in both directions and a window hub.
"""
import numpy as np
import torch

from hydra_gnn_amd import workloads
from hydra_gnn_amd.data import HeteroData, collate

OO = ("objects", "objects_to_objects", "objects")
RR = ("rooms", "rooms_to_rooms", "rooms")
O2R = ("objects", "objects_to_rooms", "rooms")
R2O = ("rooms", "rooms_to_objects", "objects")
MP3D_EDGE_TYPES = [OO, RR, O2R, R2O]   # hydra_gnn_amd/data.py:EDGE_TYPES (the conv order of a layer)
MP3D_IN_DIMS = {"objects": 306, "rooms": 6}


def cdiv(a, b):
    return (a + b - 1) // b


# =================================================================================================
# dispatch mirror
# =================================================================================================
def fpad(f):  # net.hip:fpad
    return (f + 3) // 4 * 4


def pick_shape(F, vec=4):  # aggregate.hip:pick_shape -> (GS, NV)
    lanes = cdiv(F, vec)
    gs = 8
    while gs < 64 and gs < lanes:
        gs *= 2
    return gs, cdiv(lanes, gs)


# aggregate.hip:HMP_DISPATCH_GS_NV -- the (GS, NV) instantiations of agg_fwd_kernel / agg_bwd_kernel / segment_mean_*_kernel
AGG_SHAPES = {(8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 3), (64, 4)}
PROJ_GS = {16, 32, 64}  # aggregate.hip:agg_proj_fwd_launch / agg_bwd_dx_launch switch (gs)
AGG_SMALL_TILES = 224   # aggregate.hip:AGG_SMALL_TILES
AGG_XCD_ROWS = 65536    # aggregate.hip:AGG_XCD_ROWS
AGG_WIN_MIN_ROWS = 16384  # aggregate.hip:AGG_WIN_MIN_ROWS
WR, WM, WIDCAP = 64, 64, 3072  # aggregate.hip: rows per window chunk, ring margin, ids staged per chunk
MAX_STACKED = 896       # aggregate.hip:agg_bwd_dx_launch kmax (net.hip: dx_fused needs ncols <= 896)


def proj_gs(Fmax):  # aggregate.hip:agg_proj_fwd_launch / agg_bwd_dx_launch
    gs = 16
    while gs < 64 and gs * 4 < Fmax:
        gs *= 2
    return gs


def fuse_small(total_nodes, wmax_bytes):  # net.hip:fuse_small (automatic mode; false whenever an aggregate-first conv exists)
    return total_nodes <= (65536 if wmax_bytes <= 65536 else 16384)


def xcd_mapping(rows_total):  # aggregate.hip:agg_fwd_launch / agg_bwd_launch (HMP_AGG_XCD unset)
    return rows_total >= AGG_XCD_ROWS


def small_launch(rows):  # aggregate.hip:agg_proj_fwd_launch / agg_bwd_dx_launch: 16-row tiles of the launch <= 224
    return sum(cdiv(r, 16) for r in rows) <= AGG_SMALL_TILES


def heavy(n_edges, n_rows):  # net.hip:forward_impl / backward: average degree > 8 asks for AggDst/TAggSrc::tile_rows = 8
    return n_edges > 8 * n_rows


def plain_tile8(gs, tile8_asked, rows_total, xcd=False, bf16_rows=False):
    """agg_fwd_kernel / agg_bwd_kernel run an entry in 8-row workgroups instead of 256 / GS rows (aggregate.hip:agg_fwd_launch):
    heavy rows, a small launch, and row groups narrow enough that 256 / GS > 8"""
    return tile8_asked and not (xcd or bf16_rows or rows_total > 16 * AGG_SMALL_TILES) and 256 // gs > 8


def win_in(F, n_rows, same_type_in, ce=False):  # aggregate.hip:agg_win_in (bf16 rows, HMP_AGG_WIN unset)
    return F == 256 and n_rows >= AGG_WIN_MIN_ROWS and same_type_in and not ce


def win_out(n_rows, same_type_out_F):  # aggregate.hip:agg_win_out: a same-type out-conv of width 256
    return n_rows >= AGG_WIN_MIN_ROWS and 256 in same_type_out_F


def win_chunk_ids(rowptrs, n_rows):
    """aggregate.hip:win_offsets: ids staged per 64-row chunk, summed over the given extents (forward: every incoming edge type
    of the entry; backward: every outgoing one); a chunk fits when the sum is <= WIDCAP"""
    starts = np.arange(0, n_rows, WR)
    ends = np.minimum(starts + WR, n_rows)
    tot = np.zeros(len(starts), dtype=np.int64)
    for rp in rowptrs:
        rp = np.asarray(rp)
        tot += rp[ends] - rp[starts]
    return tot


def rowptr_of(index, n):
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum(np.bincount(np.asarray(index), minlength=n))
    return rp


# ---- the launches of HeterogeneousNetwork(GraphSAGE) on the mp3d schema ----------------------------------------------
def hetero_sage_layout(hidden, out_dim, layers):
    """per layer: out widths per node type (live types only), next-layer input width, and the stacked widths (LayerLayout::ncols,
    net.hip): [one fpad(f_out) block per live conv sourced from t] + [root block if t has live in-convs].  The last layer keeps
    only the convs into the readout type (rooms): the final object states are ignored."""
    out = []
    for l in range(layers):
        last = l == layers - 1
        live = [et for et in MP3D_EDGE_TYPES if not last or et[2] == "rooms"]
        F = {}
        for et in live:
            F[et[2]] = fpad(out_dim if last else hidden)
        ncols = {t: 0 for t in ("objects", "rooms")}
        for et in live:
            ncols[et[0]] += F[et[2]]
        for t in F:
            ncols[t] += F[t]
        dim = {t: (MP3D_IN_DIMS[t] if l == 0 else hidden) for t in ("objects", "rooms")}
        out.append(dict(F=F, ncols=ncols, dim=dim, live=live))
    return out


def hetero_sage_launches(hidden, out_dim, layers, fuse, n_nodes, n_edges, ce=False):
    """the aggregation launches of one forward + backward (net.hip:forward_impl / backward; aggregate.hip:*_launch), each a dict
    kernel, gs, nv, layer and the extras: ce (masked cross entropy in the epilogue), tile8 (some entry runs 8-row tiles),
    pK / pncols (fused projection).  n_nodes: {type: rows}, n_edges: {edge type: edges}.  fuse: HMP_FUSE (None = automatic).
    Every conv is taken as projected first.  At sizes where the engine evaluates a conv aggregate-first (engine.py:
    _decide_agg_first, >= 32 768 source rows) net.hip:fuse_small returns false and the launch sequence differs: fuse=None is
    only right below that size, and the mirror does not model aggregate-first launches."""
    lay = hetero_sage_layout(hidden, out_dim, layers)
    if fuse is None:
        wmax = max(lay[l]["ncols"][t] * fpad(lay[l]["dim"][t]) * 4 for l in range(1, layers) for t in n_nodes)
        fuse = fuse_small(sum(n_nodes.values()), wmax)
    res = []
    for l in range(layers):
        Y = lay[l]
        ent = [t for t in ("objects", "rooms") if t in Y["F"] and n_nodes[t]]
        Fmax = max(Y["F"][t] for t in ent)
        asked = {t: fuse and any(heavy(n_edges[et], n_nodes[t]) for et in Y["live"] if et[2] == t) for t in ent}
        nxt = lay[l + 1] if l + 1 < layers else None
        proj = fuse and nxt is not None and all(nxt["dim"][t] % 16 == 0 and nxt["dim"][t] <= 256 for t in ent if nxt["ncols"][t]) \
            and Fmax <= 256
        if proj:
            sl = small_launch([n_nodes[t] for t in ent])
            res.append(dict(kernel="agg_proj_fwd_kernel", gs=proj_gs(Fmax), nv=1, layer=l, ce=False,
                            tile8=any(asked[t] for t in ent) and sl,
                            pK={t: nxt["dim"][t] for t in ent if nxt["ncols"][t]}, pncols={t: nxt["ncols"][t] for t in ent if nxt["ncols"][t]}))
        else:
            gs, nv = pick_shape(Fmax)
            rows_total = sum(n_nodes[t] for t in ent)  # of this launch
            tile8 = any(plain_tile8(gs, asked[t], rows_total, xcd_mapping(rows_total)) for t in ent)
            ce_here = ce and l == layers - 1 and fuse and Y["F"].get("rooms", 1 << 30) <= 256
            res.append(dict(kernel="agg_fwd_kernel", gs=gs, nv=nv, layer=l, ce=ce_here, tile8=tile8))
    for l in range(layers - 1, -1, -1):
        Y = lay[l]
        src = [t for t in ("objects", "rooms") if Y["ncols"][t] and n_nodes[t]]
        Fmax = 0
        for s in src:
            for et in Y["live"]:
                if et[0] == s:
                    Fmax = max(Fmax, Y["F"][et[2]])
            if s in Y["F"]:
                Fmax = max(Fmax, Y["F"][s])
        asked = {s: fuse and any(heavy(n_edges[et], n_nodes[s]) for et in Y["live"] if et[0] == s) for s in src}
        dx = fuse and l > 0 and all(Y["ncols"][s] <= MAX_STACKED for s in src) and Fmax <= 256
        if dx:
            sl = small_launch([n_nodes[s] for s in src])
            res.append(dict(kernel="agg_bwd_dx_kernel", gs=proj_gs(Fmax), nv=1, layer=l, ce=False, tile8=any(asked.values()) and sl))
        else:
            gs, nv = pick_shape(Fmax)
            rows_total = sum(n_nodes[s] for s in src)
            tile8 = any(plain_tile8(gs, asked[s], rows_total, xcd_mapping(rows_total)) for s in src)
            res.append(dict(kernel="agg_bwd_kernel", gs=gs, nv=nv, layer=l, ce=False, tile8=tile8))
    return res


def batch_sizes(batch):
    return ({t: int(batch[t].x.size(0)) for t in ("objects", "rooms")},
            {et: int(batch[et].edge_index.size(1)) for et in MP3D_EDGE_TYPES})


# =================================================================================================
# the degree-regime scene
# =================================================================================================
DEG_CLASSES = [0, 1, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 64, 65]
HUB = 320


def _regime_edges(rng, n_src, n_dst, same, dst_deg, src_deg, quiet, dupes=False, selfs=False, ord_deg=(0, 4)):
    """edge_index [2, E] of one edge type.  Destinations 0 .. len(dst_deg)-1 receive exactly dst_deg[i] edges (sources drawn,
    distinct, from the ordinary sources); sources S0 .. S0+len(src_deg)-1 (S0 = 32 for a same-type list, else 0) send exactly
    src_deg[k] edges into the ordinary destinations; every ordinary destination gets ord_deg[0] .. ord_deg[1]-1 edges from ordinary
    sources, and the
    `quiet` last sources send nothing.  dupes: a repeated edge in ordinary rows; selfs: j == i edges."""
    nD = len(dst_deg)
    s0 = 32 if same else 0
    S_B = np.arange(s0, s0 + len(src_deg))
    ord_src = np.array([j for j in range(n_src - quiet) if not (s0 <= j < s0 + len(src_deg))])
    ord_dst = np.arange(nD, n_dst)
    src, dst = [], []
    for i, k in enumerate(dst_deg):
        s = rng.choice(ord_src, size=k, replace=False)
        src.append(s); dst.append(np.full(k, i))
    for k, j in zip(src_deg, S_B):
        d = rng.choice(ord_dst, size=k, replace=False)
        src.append(np.full(k, j)); dst.append(d)
    for i in ord_dst:
        k = int(rng.integers(*ord_deg))
        s = rng.choice(ord_src, size=k)
        if selfs and i % 7 == 0 and i < n_src - quiet and i not in S_B:
            s = np.concatenate([s, [i]])
        if dupes and i % 5 == 0 and k:
            s = np.concatenate([s, s[:1]])
        src.append(s); dst.append(np.full(len(s), i))
    ei = np.stack([np.concatenate(src), np.concatenate(dst)]).astype(np.int64)
    return torch.from_numpy(ei[:, rng.permutation(ei.shape[1])])


def sage_regime_scene(rng, n_obj=800, n_rooms=360):
    """one mp3d-schema scene (objects 306-d = pos | size | semantic, rooms 6-d, the four edge types).  Per edge type, the first
    15 destinations have in-degree 0, 1, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 64, 65 and HUB, the 16th none; 15 sources have the
    same out-degrees (a fan-out hub among them) and the last 3 sources none.  The two lists into one node type run in opposite
    order over those destinations, so the same row is empty in one list of a pair while its partner is long (object 0: no
    objects_to_objects edge, only rooms; object 14: the reverse), and destination 15 receives nothing at all (an empty room, an
    isolated object).  objects_to_objects holds duplicate edges and self loops."""
    assert n_rooms >= HUB + 40 and n_obj >= 2 * HUB
    dst_a = DEG_CLASSES + [HUB, 0]
    dst_b = [HUB] + DEG_CLASSES[::-1][:-1] + [0, 0]  # position by position: 0 <-> HUB, 1 <-> 65, ..., HUB <-> 0, 0 <-> 0
    outs = DEG_CLASSES + [HUB]
    n = {"objects": n_obj, "rooms": n_rooms}
    # (edge type: destination degrees, dupes, self loops, ordinary in-degrees); rooms -> objects and objects -> rooms average more
    # than 8 edges per room, so both directions of a small launch cut the room entries into 8-row tiles
    spec = {OO: (dst_a, True, True, (0, 4)), R2O: (dst_b, False, False, (2, 7)), RR: (dst_a, False, False, (0, 4)),
            O2R: (dst_b, False, False, (6, 15))}
    g = HeteroData()

    def feats(k, sem):
        pos = rng.normal(0.0, 5.0, size=(k, 3))
        cols = [pos, rng.uniform(0.1, 2.0, size=(k, 3))] + ([rng.normal(0.0, 0.15, size=(k, 300))] if sem else [])
        return torch.from_numpy(np.concatenate(cols, 1).astype(np.float32)), torch.from_numpy(pos.astype(np.float32))

    g["objects"].x, g["objects"].pos = feats(n_obj, True)
    g["objects"].y = torch.from_numpy(rng.integers(0, 28, size=n_obj).astype(np.int64))
    g["rooms"].x, g["rooms"].pos = feats(n_rooms, False)
    g["rooms"].y = torch.from_numpy(rng.integers(0, workloads.NUM_ROOM_LABELS, size=n_rooms).astype(np.int64))
    for et in MP3D_EDGE_TYPES:
        deg, dupes, selfs, od = spec[et]
        g[et].edge_index = _regime_edges(rng, n[et[0]], n[et[2]], et[0] == et[2], deg, outs, 3, dupes, selfs, od)
    return g


def regime_batch(copies=1, seed=4242):
    """`copies` regime scenes and one mp3d_like_graph, collated"""
    rng = np.random.default_rng(seed)
    graphs = [sage_regime_scene(rng) for _ in range(copies)] + [workloads.mp3d_like_graph(rng)]
    return collate(graphs)


def check_sage_regimes(batch):
    """the collated batch really has what sage_regime_scene promises, per edge type and in both directions"""
    n = {t: int(batch[t].x.size(0)) for t in ("objects", "rooms")}
    want = set(DEG_CLASSES)
    deg = {}
    for et in MP3D_EDGE_TYPES:
        ei = batch[et].edge_index
        din = torch.bincount(ei[1], minlength=n[et[2]])
        dout = torch.bincount(ei[0], minlength=n[et[0]])
        deg[et] = din
        for what, d in (("in", din), ("out", dout)):
            have = set(d.tolist())
            assert want <= have, f"{et[1]} {what}-degrees: missing {sorted(want - have)}"
            assert int(d.max()) >= 300, f"{et[1]}: no {what}-degree hub"
    for a, b in ((OO, R2O), (RR, O2R)):  # an empty list of a pair beside a long partner, both ways
        assert bool(((deg[a] == 0) & (deg[b] >= 64)).any()) and bool(((deg[b] == 0) & (deg[a] >= 64)).any()), (a[1], b[1])
    assert bool(((deg[RR] == 0) & (deg[O2R] == 0)).any()), "no empty room"
    assert bool(((deg[OO] == 0) & (deg[R2O] >= 1)).any()), "no object whose only neighbour is a room"
    ei = batch[OO].edge_index
    assert bool((ei[0] == ei[1]).any()), "no self loop"
    assert int(torch.unique(ei[0] * n["objects"] + ei[1]).numel()) < ei.size(1), "no duplicate edge"
    return deg


def homogeneous_regime_graph(rng, n=800):
    """one homogeneous graph (x 6-d, one edge list): in- and out-degree classes as sage_regime_scene's objects_to_objects, and
    node 15 plus the other room_mask rows spread over the degree classes"""
    ei = _regime_edges(rng, n, n, True, DEG_CLASSES + [HUB, 0], DEG_CLASSES + [HUB], 3, True, True)
    x = torch.from_numpy(np.concatenate([rng.normal(0, 3.0, size=(n, 3)), rng.uniform(0.1, 3.0, size=(n, 3))], 1).astype(np.float32))
    room_mask = torch.zeros(n, dtype=torch.bool)
    room_mask[:16] = True
    room_mask[32:48] = True
    room_mask[rng.choice(np.arange(100, n), 40, replace=False)] = True
    return x, ei, room_mask


# =================================================================================================
# the LDS-window graph
# =================================================================================================
WIN_N_OBJ = 40_000 + 37   # n_obj % 64 != 0: the last chunk is partial
WIN_RUN_IN = (1024, 1024 + 192)    # objects whose objects_to_objects in-degree is raised to >= 76 (3 chunks over WIDCAP)
WIN_RUN_OUT = (8192, 8192 + 192)   # objects whose out-degree is raised by 60 (3 chunks over WIDCAP in the backward pass)
WIN_HUB = 20_000                   # 2400 extra in-neighbours: half within +-64 rows (inside the ring), half anywhere; the other 63
                                   # rows of its chunk lose their objects_to_objects in-edges, so the chunk fits (staged in LDS)
WIN_LONG = (25_000, 25_001, 25_002)  # +90 in-neighbours each (45 near, 45 far) in an ordinary chunk that fits
WIN_FAN = 30_000                   # sends 1500 extra edges
WIN_LONELY = (12_000, 12_100)      # no objects_to_objects in-edge: the room is the only neighbour


def window_graph(seed=31, n_obj=WIN_N_OBJ, n_rooms=400):
    g = workloads.big_hetero_graph(n_obj=n_obj, n_rooms=n_rooms, seed=seed)
    rng = np.random.default_rng(seed + 1)
    ei = g[OO].edge_index.numpy()
    src, dst = [ei[0]], [ei[1]]

    def near(rows, k, span=WM):
        r = np.repeat(rows, k)
        return np.clip(r + rng.integers(-span, span + 1, size=r.size), 0, n_obj - 1)

    rows = np.arange(*WIN_RUN_IN)   # 30 near + 30 far each: every row of the run has > 64 neighbours
    dst += [np.repeat(rows, 30), np.repeat(rows, 30)]
    src += [near(rows, 30), rng.integers(0, n_obj, size=30 * rows.size)]
    rows = np.arange(*WIN_RUN_OUT)
    src += [np.repeat(rows, 30), np.repeat(rows, 30)]
    dst += [near(rows, 30), rng.integers(0, n_obj, size=30 * rows.size)]
    src += [near(np.array([WIN_HUB]), 1200), rng.integers(0, n_obj, size=1200)]
    dst += [np.full(2400, WIN_HUB)]
    rows = np.array(WIN_LONG)
    src += [near(rows, 45), rng.integers(0, n_obj, size=45 * rows.size)]
    dst += [np.repeat(rows, 45), np.repeat(rows, 45)]
    src += [np.full(1500, WIN_FAN)]
    dst += [rng.integers(0, n_obj, size=1500)]
    s, d = np.concatenate(src), np.concatenate(dst)
    h0 = WIN_HUB // WR * WR  # the hub's chunk: only the hub keeps its objects_to_objects in-edges
    keep = ~((d >= WIN_LONELY[0]) & (d < WIN_LONELY[1])) & ~((d >= h0) & (d < h0 + WR) & (d != WIN_HUB))
    order = rng.permutation(int(keep.sum()))
    g[OO].edge_index = torch.from_numpy(np.stack([s[keep][order], d[keep][order]]).astype(np.int64))
    return g


def check_window_graph(g):
    """the window graph has chunks that fit and chunks that do not, in both directions (aggregate.hip:win_offsets); over-capacity
    chunks and chunks that fit both hold rows of more than 64 ids (a list walked 64 ids at a time from global memory / from the
    staged ids); the hub's chunk fits and about half of the hub's neighbours lie inside the ring rows of that chunk (the chunk
    plus WM rows either side), the rest outside; the fan-out exists; lonely objects have only their room.
    Forward, the objects entry stages objects_to_objects and rooms_to_objects; backward, objects_to_objects only (the
    objects -> rooms conv is evaluated aggregate-first at this size: its block is gathered on the rooms side)."""
    n = int(g["objects"].x.size(0))
    assert n % WR != 0 and n >= AGG_WIN_MIN_ROWS
    oo = g[OO].edge_index.numpy()
    r2o = g[R2O].edge_index.numpy()
    fwd = win_chunk_ids([rowptr_of(np.sort(oo[1]), n), rowptr_of(np.sort(r2o[1]), n)], n)
    bwd = win_chunk_ids([rowptr_of(np.sort(oo[0]), n)], n)
    din = np.bincount(oo[1], minlength=n)
    dout = np.bincount(oo[0], minlength=n)
    for what, ids in (("forward", fwd), ("backward", bwd)):
        assert (ids <= WIDCAP).sum() > 100 and (ids > WIDCAP).sum() >= 2, (what, int((ids > WIDCAP).sum()))
    over_f = np.nonzero(fwd > WIDCAP)[0]
    assert any(din[c * WR:(c + 1) * WR].max() > 64 for c in over_f), "no row of > 64 ids in an over-capacity forward chunk"
    over_b = np.nonzero(bwd > WIDCAP)[0]
    assert any(dout[c * WR:(c + 1) * WR].max() > 64 for c in over_b), "no row of > 64 ids in an over-capacity backward chunk"
    hc = WIN_HUB // WR
    fit_f = np.nonzero(fwd <= WIDCAP)[0]
    assert any(din[c * WR:(c + 1) * WR].max() > 64 for c in fit_f if c != hc), "no long row in an ordinary fitting forward chunk"
    fit_b = np.nonzero(bwd <= WIDCAP)[0]
    assert any(dout[c * WR:(c + 1) * WR].max() > 64 for c in fit_b), "no row of > 64 ids in a fitting backward chunk"
    hub_src = oo[0][oo[1] == WIN_HUB]
    assert hub_src.size >= 2000
    assert fwd[hc] <= WIDCAP, ("the hub's chunk does not fit", int(fwd[hc]))
    r_c = hc * WR
    in_ring = (hub_src >= max(r_c - WM, 0)) & (hub_src < min(r_c + WR + WM, n))  # agg_fwd_win_kernel: wlo / whi of the chunk
    assert 0.3 < float(in_ring.mean()) < 0.7, ("hub: not about half inside the ring", float(in_ring.mean()))
    assert dout[WIN_FAN] >= 1500
    lonely = np.arange(*WIN_LONELY)
    assert (din[lonely] == 0).all() and (np.bincount(r2o[1], minlength=n)[lonely] == 1).all()
    return fwd, bwd


# =================================================================================================
# the cases of tests/test_gpu_sage_kernels.py (tests/test_sage_dispatch.py checks what they reach)
# =================================================================================================
HIDDEN_CASES = [32, 48, 64, 128, 208, 256, 300, 512, 768, 1000]  # x HMP_FUSE in {0, 1}, output 26, on regime_batch()
UNSUPPORTED_HIDDEN = 1025          # fpad = 1028 > 64 lanes x 4 chunks x 4 floats
CE_OUT_DIMS = [26, 40, 100, 200]   # fused training step (HMP_FUSE=1), hidden CE_HIDDEN
CE_HIDDEN = 64
DROPOUT_HIDDEN = [64, 256]         # training mode, dropout 0.25: GS 16 and GS 64
LAUNCH_COPIES = [1, 10]            # regime scenes per batch: 8-row tiles / none (HMP_FUSE=1, hidden LAUNCH_HIDDEN)
LAUNCH_HIDDEN = 64
# hmp_segment_mean_fwd / _bwd: (F, extra columns of the input's leading dimension, of the output's); an odd leading dimension
# or F % 4 != 0 takes the VEC = 1 kernels, F > 1024 two column panels
SEGMENT_CASES = [(28, 0, 4), (64, 0, 4), (128, 4, 8), (256, 0, 4), (300, 4, 4), (768, 0, 4), (1000, 0, 4), (1100, 0, 4), (64, 3, 1), (30, 2, 2)]


def segment_shape(F, pad_in, pad_out):
    """(GS, NV, VEC) of every column panel hmp_segment_mean_* launches (aggregate.hip:hmp_segment_mean_fwd / segment_mean_dispatch)"""
    vec_ok = (F + pad_in) % 4 == 0 and (F + pad_out) % 4 == 0 and F % 4 == 0
    panel = 1024 if vec_ok else 256
    out = []
    for c in range(0, F, panel):
        w = min(panel, F - c)
        v = 4 if vec_ok else 1
        out.append(pick_shape(w, v) + (v,))
    return out


def case_launches():
    """every aggregation launch of the GPU cases: (case, launch dict)"""
    b1 = regime_batch()
    nn, ne = batch_sizes(b1)
    res = []
    for h in HIDDEN_CASES:
        for fuse in (False, True):
            res += [(("hidden", h, fuse), d) for d in hetero_sage_launches(h, 26, 3, fuse, nn, ne)]
    for o in CE_OUT_DIMS:
        res += [(("ce", o), d) for d in hetero_sage_launches(CE_HIDDEN, o, 3, True, nn, ne, ce=True)]
    for copies in LAUNCH_COPIES:
        b = b1 if copies == 1 else regime_batch(copies)
        n2, e2 = batch_sizes(b)
        res += [(("launch", copies), d) for d in hetero_sage_launches(LAUNCH_HIDDEN, 26, 3, True, n2, e2)]
    return res
