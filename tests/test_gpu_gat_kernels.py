"""K3 (csrc/gat.hip) at the shapes and edges that test_gpu_gat.py does not reach.

Unit level (hmp_gat_fwd + hmp_gat_bwd against a float64 restatement):
  * every heads-class x row-group instantiation (HM in {1, 2, 4, 8} x GS in {8, 16, 32, 64}), heads 5..7 included;
  * destination rows of 0, 1, UB-1, UB, UB+1, 31, 32, 33, 64, 65 slots and a hub of thousands in one graph: backward pass 1
    parks the first 32 slots of a row in LDS and recomputes the rest, so rows past 32 slots run a second code path;
  * a source hub of out-degree > 1000 and sources without out-edges (backward pass 2, CSC), duplicate edges;
  * removed self loops (explicit j == i with self_loops = 1) at slot 0, 31, 32 and past 32 of a row;
  * edge attributes of every width, attention dropout on heads 0..3 and 4..7 (the second hash word);
  * logits of +-100 (plain exp overflows fp32), rows of equal logits, rows whose maximum is the appended loop;
  * strided operands and a gradient that is strided or 4-byte offset, so C % 4 == 0 also runs the element-wise path;
  * every output starts as NaN: each documented element must be written, everything outside the documented region
    must keep its NaN; two identical calls must agree bit for bit.
Network level: the same regimes through the executor (head mean, bias + ELU + feature dropout, two edge types into one
destination), on scene graphs with rooms of 0 .. 150 objects and an object hub.

Tolerance: 1e-5 (atol + rtol) against float64, as in test_gpu_gat.py.
"""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hydra_gnn_amd import _lib, workloads  # noqa: E402
from hydra_gnn_amd.data import Data, HeteroData, collate, compute_relative_pos  # noqa: E402
from hydra_gnn_amd.models import HomogeneousNetwork  # noqa: E402
from oracle import models as omodels  # noqa: E402
from test_gpu_gat import check_model, gat_pair, training_mode_parity  # noqa: E402
from test_gpu_ops import build_plan  # noqa: E402

ATOL, RTOL = 1e-5, 1e-5
DEV = "cuda:0"
HMAX = 8     # GAT_HMAX: per-row / per-edge scalars are stored [*, 8]
CAP = 32     # slots per row whose backward-pass-1 scalars live in LDS (gat_bwd1_kernel)
NAN = float("nan")


def align4(c):
    return (c + 3) // 4 * 4


def unroll(H):
    """neighbour slots per fetch batch (UB in gat.hip): 4 up to 4 heads, 2 for heads-class 8"""
    return 4 if H <= 4 else 2


def dispatch_class(H, C):
    """(heads-class, row-group width) the launch picks (gat.hip dispatch())"""
    hm = 1 if H <= 1 else 2 if H <= 2 else 4 if H <= 4 else 8
    gs = 8
    while gs < 64 and gs < align4(C) // 4:
        gs *= 2
    return hm, gs


# =================================================================================================
# graphs
# =================================================================================================
def regime_graph(seed, n_src, n_dst, loops, ub, hub, fan):
    """edge_index [2, E] whose destination rows 0..9 have 1, ub-1, ub, ub+1, 31, 32, 33, 64, 65 and `hub` slots (a slot is a
    CSR entry, removed self loops included, or the appended loop), rows 10.. up to 2 random edges, the last row none.
    Explicit self loops sit at slot 31 of the 33-slot row, 32 and 63 of the 64-slot row, 0, 31, 32 and 40 of the 65-slot row and
    twice in the hub row; the 31-slot row repeats three edges.  Source 12 is a hub: one edge into each of the `fan` rows after
    the regime rows.  The last two sources send no edge.  The edges are shuffled, the order within a row is the one built here.
    (The hubs draw distinct rows / mostly distinct sources: thousands of copies of one term would make an fp32 sum drift by
    up to n * 2^-24 of its size, the fp32 bound for n same-sign terms, past the 1e-5 tolerance.)"""
    assert min(n_src, n_dst) >= 16 and n_dst >= 11 + fan
    rng = np.random.default_rng(seed)
    n_loop = min(n_src, n_dst) if loops else 0
    s_hub, quiet = 12, {n_src - 1, n_src - 2}
    pool = np.array([j for j in range(n_src) if j not in quiet and j != s_hub])
    slots = [1, ub - 1, ub, ub + 1, 31, 32, 33, 64, 65, hub]
    selfs = {6: [31], 7: [32, 63], 8: [0, 31, 32, 40], 9: [100, hub - 2]}  # row -> slot indices holding j == i
    lists = []
    for r in range(n_dst):
        if r < len(slots):
            k = max(slots[r] - (1 if r < n_loop else 0), 0)
        elif r == n_dst - 1:
            k = 0
        else:
            k = int(rng.integers(0, 3))
        src = rng.choice(pool, size=k)
        if len(slots) <= r < len(slots) + fan:
            src = np.concatenate([[s_hub], src])
        if r == 4:  # the 31-slot row: three edges repeated
            src[3:6] = src[0:3]
        for q in selfs.get(r, []):
            if q < k:
                src[q] = r
        lists.append(src)
    rows = np.concatenate([np.full(len(s), r) for r, s in enumerate(lists)]).astype(np.int64)
    rng.shuffle(rows)
    src = np.empty_like(rows)
    src[np.argsort(rows, kind="stable")] = np.concatenate(lists).astype(np.int64)
    return torch.from_numpy(np.stack([src, rows]))


def regime_case(seed, H, C, geometry, loops, budget=4_500_000):
    """regime_graph sized for H x C: a destination hub of up to 3000 slots and a source hub of up to 1100 out-edges, capped so
    the float64 reference gathers at most ~`budget` elements.  geometry: n_src == n_dst, n_src < n_dst or n_src > n_dst.
    Returns ei, n_src, n_dst."""
    slots = min(7000, budget // (H * C))
    hub, fan = min(3000, int(0.45 * slots)), min(1100, int(0.2 * slots))
    n = fan + 24
    n_src, n_dst = {"eq": (n, n), "src<dst": (n - 8, n), "src>dst": (n + 8, n)}[geometry]
    ei = regime_graph(seed, n_src, n_dst, loops, unroll(H), hub, fan)
    check_regimes(ei, n_src, n_dst, loops, unroll(H), hub, fan)
    return ei, n_src, n_dst


def slot_counts(ei, n_src, n_dst, loops):
    n_loop = min(n_src, n_dst) if loops else 0
    cnt = torch.bincount(ei[1], minlength=n_dst)
    cnt[:n_loop] += 1
    return cnt


def slot_index(ei):
    """index of every original edge inside its destination row (CSR order = stable sort by destination)"""
    E = ei.size(1)
    order = torch.sort(ei[1], stable=True).indices
    pos_of = torch.empty(E, dtype=torch.int64)
    pos_of[order] = torch.arange(E)
    first = torch.zeros(int(ei[1].max()) + 2 if E else 1, dtype=torch.int64)
    if E:
        first[1:] = torch.cumsum(torch.bincount(ei[1], minlength=first.numel() - 1), 0)
        return pos_of, pos_of - first[ei[1]]
    return pos_of, pos_of


# =================================================================================================
# float64 reference
# =================================================================================================
def gat_reference_full(h, a_s, a_d, ea, ve, ei, n_dst, self_loops, gout, keep=None, p=0.0):
    """float64 GATConv steps 3-7 for given projected inputs, differentiated by autograd on the RAW logits.
    Returns out [n_dst, H, C], smax / sden [n_dst, H] (row max of the leaky logits, sum exp(e - max) + 1e-16), alpha after
    dropout and d loss / d raw logit per CSR position [E + n_loop, H] (loops at E + i, removed self loops 0) and
    d loss / d raw logit in original edge order [E, H]; loss = <out, gout>.  The gradients land in the leaves' .grad.
    keep [E + n_loop, >= H]: keep flags by CSR position (None: no dropout)."""
    n_src, H, C = h.shape
    E = ei.size(1)
    n_loop = min(n_src, n_dst) if self_loops else 0
    pos_of, _ = slot_index(ei)
    live = torch.nonzero(ei[0] != ei[1] if self_loops else torch.ones(E, dtype=torch.bool)).flatten()
    loop = torch.arange(n_loop)
    j = torch.cat([ei[0, live], loop])
    i = torch.cat([ei[1, live], loop])
    pos = torch.cat([pos_of[live], E + loop])
    raw = a_s[j] + a_d[i]
    if ea is not None and ve is not None:
        raw = raw + torch.cat([ea[live] @ ve, ve.new_zeros(n_loop, H)], 0)
    raw.retain_grad()
    e = torch.nn.functional.leaky_relu(raw, 0.2)
    idx = i.unsqueeze(1).expand(-1, H)
    m = torch.full((n_dst, H), -torch.inf, dtype=e.dtype).scatter_reduce(0, idx, e.detach(), "amax", include_self=True)
    ex = torch.exp(e - m[i])
    s = torch.zeros(n_dst, H, dtype=e.dtype).index_add(0, i, ex)
    alpha = ex / (s + 1e-16)[i]
    if keep is not None:
        alpha = alpha * keep[pos, :H].to(alpha.dtype) / (1.0 - p)
    out = torch.zeros(n_dst, H, C, dtype=h.dtype).index_add(0, i, alpha.unsqueeze(-1) * h[j])
    (out * gout.reshape(n_dst, H, C)).sum().backward()
    ap = torch.zeros(E + n_loop, H, dtype=h.dtype)
    dl = torch.zeros(E + n_loop, H, dtype=h.dtype)
    ap[pos] = alpha.detach()
    dl[pos] = raw.grad
    dlo = torch.zeros(E, H, dtype=h.dtype)
    dlo[live] = raw.grad[: live.numel()]
    return dict(out=out.detach(), smax=m, sden=s.detach() + 1e-16, alpha_drop=ap, dlogit=dl, dlogit_orig=dlo)


# =================================================================================================
# unit runner
# =================================================================================================
# operand layouts.  dense: the executor's (16-byte aligned rows, a / g-a at stride 8).  strided: every leading dimension
# padded, the gradient's ld % 4 == 1.  offset: tight a / g-a strides (== H), the gradient's base 4 bytes past a 16-byte
# boundary.  strided and offset run the element-wise gradient path of both backward passes even when C % 4 == 0.
LAYOUTS = {
    "dense": dict(ldh=0, las=HMAX, lad=HMAX, ldo=None, g="dense", ldgh=0, lgas=HMAX, lgad=HMAX),
    "strided": dict(ldh=8, las=11, lad=9, ldo=5, g="odd", ldgh=12, lgas=13, lgad=10),
    "offset": dict(ldh=4, las=0, lad=0, ldo=0, g="offset", ldgh=0, lgas=0, lgad=0),
}


def grid(rng, lo, hi, size):
    """uniform on a 1/64 grid: sums and products of a few of these are exact in fp32"""
    return torch.from_numpy(np.round(rng.uniform(lo, hi, size=size) * 64.0) / 64.0).float()


def make_values(rng, values, n_src, n_dst, H, C, E, edim):
    f = lambda *s: torch.from_numpy(rng.normal(0, 1, size=s).astype(np.float32))
    h = f(n_src, H, C)
    if values == "normal":
        a_s, a_d = f(n_src, H), f(n_dst, H)
        ea, ve = f(E, edim), 0.5 * f(edim, H)
    elif values == "wide":       # raw logits up to +-(50 + 50 + 4 * 4): exp overflows fp32 past 88.7
        a_s, a_d = grid(rng, -50, 50, (n_src, H)), grid(rng, -50, 50, (n_dst, H))
        ea, ve = grid(rng, -2, 2, (E, edim)), grid(rng, -2, 2, (edim, H))
    elif values == "uniform":    # every logit of a row equal: alpha = 1 / slots
        a_s, a_d = torch.full((n_src, H), 0.75), f(n_dst, H)
        ea, ve = f(E, edim), torch.zeros(edim, H)
    elif values == "loop_max":   # real edges carry an edge term <= -48, the loop 0: the row maximum is the last slot
        assert edim >= 1
        a_s, a_d = grid(rng, -2, 2, (n_src, H)), grid(rng, -2, 2, (n_dst, H))
        ea = grid(rng, 1.0, 2.0, (E, edim))
        ve = torch.zeros(edim, H)
        ve[0] = -48.0
    else:
        raise ValueError(values)
    return h, a_s, a_d, (ea if edim else None), (ve if edim else None)


def run_unit(H, Cc, ei, n_src, n_dst, loops, edim=0, p=0.0, values="normal", layout="dense", seed=0):
    """hmp_gat_fwd + hmp_gat_bwd on poisoned, laid-out buffers; every output checked against gat_reference_full, every
    element outside the documented regions checked to be untouched, and a second run checked to be bitwise equal."""
    lib = _lib.require_device()
    rng = np.random.default_rng(seed)
    E = ei.size(1)
    Cp = align4(Cc)
    HC, HCp = H * Cc, H * Cp
    n_loop = min(n_src, n_dst) if loops else 0
    P = E + n_loop
    L = LAYOUTS[layout]
    ldh = HCp + L["ldh"]
    las, lad = L["las"] or H, L["lad"] or H
    ldo = HC + (L["ldo"] if L["ldo"] is not None else (align4(HC) - HC))
    ldgh = HCp + L["ldgh"]
    lgas, lgad = L["lgas"] or H, L["lgad"] or H
    ldg = align4(HC) + (1 if L["g"] == "odd" else 0)

    plan = build_plan(ei.to(DEV), n_src, n_dst)
    assert plan["status"] == 0
    h, a_s, a_d, ea, ve = make_values(rng, values, n_src, n_dst, H, Cc, E, edim)
    gout = torch.from_numpy(rng.normal(0, 1, size=(n_dst, HC)).astype(np.float32))
    if E:
        # backward pass 2 sums the n out-edges of a source in fp32, in edge order: with g ~ N(0, 1) the partial sums of the source
        # hub reach ~sqrt(n) and their rounding alone ~1e-5.  The gradient rows it reaches are scaled by 1 / sqrt(n), so its sum
        # stays O(1) and its rounding O(sqrt(n) * 2^-24), well inside the tolerance.
        out_deg = torch.bincount(ei[0], minlength=n_src)
        if int(out_deg.max()) > 256:
            gout[ei[1, ei[0] == int(out_deg.argmax())]] /= float(out_deg.max()) ** 0.5
    keep = None
    args = _lib.GatArgs(H, Cc, int(loops), edim, p, 0x5EED0000 + seed, 7, 3)
    if p > 0:
        m = torch.zeros(P * HMAX, dtype=torch.uint8, device=DEV)
        _lib.check(lib.hmp_dropout_mask(args.seed, args.rng_step, args.rng_stream, p, P, HMAX, m.data_ptr(), _lib.stream_ptr()))
        keep = m.view(P, HMAX).cpu()

    # inputs: every column the kernels must not read is NaN (the padding of h, read and multiplied by zero, is finite junk)
    h_dev = torch.full((n_src, ldh), NAN)
    hv = h_dev[:, :HCp].view(n_src, H, Cp)
    hv[:] = 3.0
    hv[:, :, :Cc] = h
    h_dev = h_dev.to(DEV)
    as_dev = torch.full((n_src, las), NAN); as_dev[:, :H] = a_s; as_dev = as_dev.to(DEV)
    ad_dev = torch.full((n_dst, lad), NAN); ad_dev[:, :H] = a_d; ad_dev = ad_dev.to(DEV)
    ea_dev = ea.contiguous().to(DEV) if ea is not None and E else None
    ve_dev = None
    if ve is not None:
        ve_dev = torch.full((edim, HMAX), NAN); ve_dev[:, :H] = ve; ve_dev = ve_dev.to(DEV)
    g_buf = torch.full((n_dst * ldg + 1,), NAN)
    g_off = 1 if L["g"] == "offset" else 0
    g_buf[g_off:g_off + n_dst * ldg].view(n_dst, ldg)[:, :HC] = gout
    g_buf = g_buf.to(DEV)
    g_ptr = g_buf.data_ptr() + 4 * g_off
    ptr = lambda t: t.data_ptr() if t is not None else None

    def call():
        o = dict(smax=torch.full((n_dst, HMAX), NAN, device=DEV), sden=torch.full((n_dst, HMAX), NAN, device=DEV),
                 out=torch.full((n_dst, ldo), NAN, device=DEV),
                 alpha_drop=torch.full((P + 2, HMAX), NAN, device=DEV), dlogit=torch.full((P + 2, HMAX), NAN, device=DEV),
                 dlogit_orig=torch.full((max(E, 1), HMAX), NAN, device=DEV),
                 g_h=torch.full((n_src, ldgh), NAN, device=DEV), g_as=torch.full((n_src, lgas), NAN, device=DEV),
                 g_ad=torch.full((n_dst, lgad), NAN, device=DEV))
        torch.cuda.synchronize()
        _lib.check(lib.hmp_gat_fwd(h_dev.data_ptr(), ldh, as_dev.data_ptr(), las, ad_dev.data_ptr(), lad, ptr(ea_dev), ptr(ve_dev),
                                   plan["plan"], args, o["smax"].data_ptr(), o["sden"].data_ptr(), o["out"].data_ptr(), ldo,
                                   _lib.stream_ptr()))
        _lib.check(lib.hmp_gat_bwd(g_ptr, ldg, h_dev.data_ptr(), ldh, as_dev.data_ptr(), las, ad_dev.data_ptr(), lad,
                                   ptr(ea_dev), ptr(ve_dev), plan["plan"], args, o["smax"].data_ptr(), o["sden"].data_ptr(),
                                   o["alpha_drop"].data_ptr(), o["dlogit"].data_ptr(), o["dlogit_orig"].data_ptr(),
                                   o["g_h"].data_ptr(), ldgh, o["g_as"].data_ptr(), lgas, o["g_ad"].data_ptr(), lgad,
                                   _lib.stream_ptr()))
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in o.items()}

    got = call()
    h64, as64, ad64 = (t.double().requires_grad_(True) for t in (h, a_s, a_d))
    ve64 = ve.double().requires_grad_(True) if ve is not None else None
    ref = gat_reference_full(h64, as64, ad64, ea.double() if ea is not None else None, ve64, ei, n_dst, loops, gout.double(),
                             keep, p)

    def close(name, a, b):
        torch.testing.assert_close(a.double(), b, atol=ATOL, rtol=RTOL, msg=lambda s: f"{name}: {s}")

    def untouched(name, t):
        assert torch.isnan(t).all(), f"{name}: an element outside the documented region was written"

    close("out", got["out"][:, :HC], ref["out"].reshape(n_dst, HC))
    untouched("out[:, H*C:]", got["out"][:, HC:])
    close("smax", got["smax"][:, :H], ref["smax"])
    close("sden", got["sden"][:, :H], ref["sden"])
    for k in ("alpha_drop", "dlogit"):
        close(k, got[k][:P, :H], ref[k])
        untouched(f"{k}[:, H:]", got[k][:, H:])
        untouched(f"{k}[E + n_loop:]", got[k][P:])
    if E:
        close("dlogit_orig", got["dlogit_orig"][:, :H], ref["dlogit_orig"])
        untouched("dlogit_orig[:, H:]", got["dlogit_orig"][:, H:])
    else:
        untouched("dlogit_orig (no edges)", got["dlogit_orig"])
    if loops and E:  # removed self loops: exactly zero, by CSR position and in original order
        pos_of, _ = slot_index(ei)
        sl = torch.nonzero(ei[0] == ei[1]).flatten()
        for k in ("alpha_drop", "dlogit"):
            assert torch.equal(got[k][pos_of[sl], :H], torch.zeros(sl.numel(), H)), f"{k}: removed self loop not 0"
        assert torch.equal(got["dlogit_orig"][sl, :H], torch.zeros(sl.numel(), H)), "dlogit_orig: removed self loop not 0"
    gh = got["g_h"][:, :HCp].reshape(n_src, H, Cp)
    close("g_h", gh[:, :, :Cc], h64.grad)
    assert torch.equal(gh[:, :, Cc:], torch.zeros(n_src, H, Cp - Cc)), "g_h: padding columns C..Cp not 0"
    untouched("g_h[:, H*Cp:]", got["g_h"][:, HCp:])
    close("g_a_src", got["g_as"][:, :H], as64.grad)
    close("g_a_dst", got["g_ad"][:, :H], ad64.grad)
    untouched("g_a_src[:, H:]", got["g_as"][:, H:])
    untouched("g_a_dst[:, H:]", got["g_ad"][:, H:])
    if ve is not None and E:
        close("g_v_edge", ea.double().t() @ got["dlogit_orig"][:, :H].double(), ve64.grad)

    again = call()  # no atomics: the same call gives the same bits, NaN padding included
    for k, v in got.items():
        assert torch.equal(v.view(torch.int32), again[k].view(torch.int32)), f"{k}: two identical calls differ"
    return dict(got=got, ref=ref, keep=keep, plan=plan)


def check_regimes(ei, n_src, n_dst, loops, ub, hub, fan):
    """the graph really has the degree classes regime_graph promises"""
    cnt = slot_counts(ei, n_src, n_dst, loops)
    have = set(cnt.tolist())
    want = {1, ub - 1, ub, ub + 1, 31, 32, 33, 64, 65}
    assert want <= have, f"missing slot counts {want - have}"
    assert int(cnt.max()) == hub > 65
    out_deg = torch.bincount(ei[0], minlength=n_src)
    assert int(out_deg.max()) >= fan and int(out_deg.min()) == 0
    assert int(torch.bincount(ei[1] * n_src + ei[0]).max()) > 1, "no duplicate edge"
    if n_dst > n_src or not loops:
        assert 0 in have


# =================================================================================================
# A.1 + A.2 + A.7 + A.8: every heads-class x row-group instantiation on the degree-regime graph
# =================================================================================================
DISPATCH_CASES = [
    # H, C, geometry, loops, edim, p, layout
    (1, 6, "src<dst", 1, 0, 0.0, "dense"),
    (1, 64, "eq", 1, 3, 0.0, "strided"),
    (1, 101, "src>dst", 1, 0, 0.25, "offset"),
    (1, 256, "eq", 0, 2, 0.0, "dense"),
    (2, 32, "eq", 1, 1, 0.0, "offset"),
    (2, 33, "src<dst", 1, 0, 0.5, "strided"),
    (2, 128, "eq", 1, 3, 0.0, "dense"),
    (2, 129, "src>dst", 0, 0, 0.0, "strided"),
    (3, 1, "eq", 1, 4, 0.0, "strided"),
    (4, 64, "eq", 1, 0, 0.25, "dense"),
    (3, 100, "src<dst", 1, 3, 0.0, "offset"),
    (4, 256, "eq", 1, 0, 0.0, "strided"),
    (8, 6, "eq", 1, 3, 0.25, "dense"),
    (5, 64, "src>dst", 1, 0, 0.0, "offset"),
    (7, 101, "eq", 0, 2, 0.0, "strided"),
    (6, 129, "eq", 1, 0, 0.0, "dense"),
    (8, 256, "src<dst", 1, 2, 0.0, "dense"),
]


def test_dispatch_cases_reach_every_instantiation():
    reached = {dispatch_class(c[0], c[1]) for c in DISPATCH_CASES}
    assert reached == {(hm, gs) for hm in (1, 2, 4, 8) for gs in (8, 16, 32, 64)}
    for hm in (1, 2, 4, 8):  # C % 4 == 0 and != 0 in every heads class
        assert {c[1] % 4 == 0 for c in DISPATCH_CASES if dispatch_class(c[0], c[1])[0] == hm} == {True, False}


@pytest.mark.parametrize("H,Cc,geometry,loops,edim,p,layout", DISPATCH_CASES,
                         ids=[f"H{c[0]}-C{c[1]}-hm{dispatch_class(c[0], c[1])[0]}-gs{dispatch_class(c[0], c[1])[1]}-{c[6]}"
                              for c in DISPATCH_CASES])
def test_gat_unit_dispatch_class_on_degree_regimes(H, Cc, geometry, loops, edim, p, layout):
    ei, n_src, n_dst = regime_case(H * 1000 + Cc, H, Cc, geometry, loops)
    run_unit(H, Cc, ei, n_src, n_dst, loops, edim=edim, p=p, layout=layout, seed=H + Cc)


@pytest.mark.parametrize("layout", ["dense", "strided", "offset"])
@pytest.mark.parametrize("H,Cc", [(4, 64), (8, 32)])
def test_gat_unit_strided_and_unaligned_operands(H, Cc, layout):
    """C % 4 == 0: the dense layout runs the 16-byte gradient loads, strided (ld % 4 != 0) and offset (base 4 bytes past 16) the
    element-wise ones; all must give the float64 results and leave every pad column NaN."""
    ei, n_src, n_dst = regime_case(77, H, Cc, "eq", 1)
    run_unit(H, Cc, ei, n_src, n_dst, 1, edim=2, layout=layout, seed=5)


# =================================================================================================
# A.2 / A.3: empty graphs, loop-only rows, removed self loops at and past the cache boundary
# =================================================================================================
@pytest.mark.parametrize("n_src,n_dst", [(5, 7), (7, 5), (6, 6)])
def test_gat_unit_no_edges_loops_only(n_src, n_dst):
    """E = 0 with self_loops = 1: every row < min(n_src, n_dst) has the loop as its only slot, the others none."""
    run_unit(2, 9, torch.zeros(2, 0, dtype=torch.int64), n_src, n_dst, 1, edim=3, layout="strided")
    run_unit(5, 12, torch.zeros(2, 0, dtype=torch.int64), n_src, n_dst, 1, p=0.5)


@pytest.mark.parametrize("geometry,loops", [("src<dst", 1), ("src>dst", 1), ("eq", 1), ("eq", 0)])
@pytest.mark.parametrize("H", [2, 8])
def test_gat_unit_removed_self_loops_across_the_cache(geometry, loops, H):
    """explicit j == i edges at slot 0, 31, 32 and > 32 of a row: removed with self_loops = 1 (alpha', d logit and the original-
    order d logit exactly 0, checked in run_unit), ordinary edges without.  n_src != n_dst leaves rows without a loop."""
    ei, n_src, n_dst = regime_case(300 + H, H, 20, geometry, loops)
    _, idx = slot_index(ei)
    sl = ei[0] == ei[1]
    have = set(idx[sl].tolist())
    assert {0, 31, 32} <= have and max(have) > CAP
    r = run_unit(H, 20, ei, n_src, n_dst, loops, edim=2, seed=H)
    if not loops:  # a kept j == i edge carries a real alpha
        pos_of, _ = slot_index(ei)
        assert (r["got"]["alpha_drop"][pos_of[sl], :H] > 0).all()


# =================================================================================================
# A.4 edge attributes, A.5 attention dropout
# =================================================================================================
@pytest.mark.parametrize("loops", [0, 1])
@pytest.mark.parametrize("edim", [1, 2, 3, 4])
def test_gat_unit_edge_attributes(edim, loops):
    ei, n_src, n_dst = regime_case(40 + edim, 3, 20, "src<dst", loops)
    run_unit(3, 20, ei, n_src, n_dst, loops, edim=edim, seed=edim, layout="strided" if edim % 2 else "dense")


@pytest.mark.parametrize("p", [0.25, 0.5])
@pytest.mark.parametrize("H", [3, 4, 6, 8])
def test_gat_unit_attention_dropout(H, p):
    """the keep flags of heads 0..3 come from the first hash word of element (pos, h), those of heads 4..7 from the second;
    rows above and below 32 slots, loops at E + i, removed self loops (never drawn for)."""
    ei, n_src, n_dst = regime_case(500 + H, H, 12, "src<dst", 1)
    r = run_unit(H, 12, ei, n_src, n_dst, 1, edim=2, p=p, seed=H)
    keep = r["keep"][:, :H]
    assert 0 < keep.float().mean() < 1
    if H > 4:
        assert (keep[:, 4:] == 0).any() and (keep[:, 4:] == 1).any()


# =================================================================================================
# A.6 logit range
# =================================================================================================
@pytest.mark.parametrize("values,edim", [("wide", 3), ("uniform", 0), ("loop_max", 1)])
@pytest.mark.parametrize("H,Cc", [(4, 24), (8, 9)])
def test_gat_unit_logit_range(H, Cc, values, edim):
    """wide: logits of +-100 on a 1/64 grid (the fp32 sums are exact, plain exp(100) is inf), so only a max-subtracted online
    softmax stays at 1e-5.  uniform: every logit of a row equal.  loop_max: the appended loop holds the row maximum, so the
    online softmax rescales at the last slot."""
    ei, n, _ = regime_case(900 + H, H, Cc, "eq", 1)
    r = run_unit(H, Cc, ei, n, n, 1, edim=edim, values=values, seed=3)
    ref = r["ref"]
    E = ei.size(1)
    if values == "wide":
        assert ref["smax"][torch.isfinite(ref["smax"])].max() > 88.7
    if values == "uniform":
        live = slot_counts(ei, n, n, 1) - torch.bincount(ei[1][ei[0] == ei[1]], minlength=n)
        torch.testing.assert_close(ref["alpha_drop"][E:], (1.0 / live.double()).unsqueeze(1).expand(-1, H), atol=1e-12, rtol=1e-12)
    if values == "loop_max":  # the loop's alpha beats every other alpha of its row
        dst_of_pos = torch.sort(ei[1], stable=True).values.unsqueeze(1).expand(-1, H)
        best = torch.zeros(n, H, dtype=torch.float64).scatter_reduce(0, dst_of_pos, ref["alpha_drop"][:E], "amax")
        assert (ref["alpha_drop"][E:] > best).all()


# =================================================================================================
# B. network level
# =================================================================================================
def regime_scene(rng, room_sizes, hub_room=None):
    """one mp3d_like_graph-schema scene (objects 306-d = pos | size | semantic, rooms 6-d = pos | size, the four edge types) with
    the given objects per room; objects_to_objects links pairs inside a room (mean in-degree ~6), and the first object of
    `hub_room` to every other object of that room, both ways."""
    n_rooms = len(room_sizes)
    per_room = np.asarray(room_sizes, dtype=np.int64)
    n_obj = int(per_room.sum())
    room_of = np.repeat(np.arange(n_rooms), per_room)
    start = np.concatenate([[0], np.cumsum(per_room)])
    pairs = []
    for r, k in enumerate(per_room):
        k = int(k)
        if k < 2:
            continue
        iu, ju = np.triu_indices(k, 1)
        sel = rng.choice(iu.size, size=min(iu.size, 3 * k), replace=False)
        if r == hub_room:
            sel = np.union1d(sel, np.nonzero(iu == 0)[0])
        pairs.append(np.stack([iu[sel], ju[sel]], 1) + start[r])
    pairs = np.concatenate(pairs, 0) if pairs else np.zeros((0, 2), dtype=np.int64)
    oo = np.concatenate([pairs.T, pairs[:, ::-1].T], 1).astype(np.int64)
    tree = np.array([[int(rng.integers(0, v)), v] for v in range(1, n_rooms)], dtype=np.int64).reshape(-1, 2)
    rr = np.concatenate([tree.T, tree[:, ::-1].T], 1).astype(np.int64)
    ro = np.stack([room_of, np.arange(n_obj)], 0).astype(np.int64)

    def feats(n, sem):
        pos = rng.normal(0.0, 5.0, size=(n, 3))
        cols = [pos, rng.uniform(0.1, 2.0, size=(n, 3))] + ([rng.normal(0.0, 0.15, size=(n, 300))] if sem else [])
        return torch.from_numpy(np.concatenate(cols, 1).astype(np.float32)), torch.from_numpy(pos.astype(np.float32))

    g = HeteroData()
    g["objects"].x, g["objects"].pos = feats(n_obj, True)
    g["objects"].y = torch.from_numpy(rng.integers(0, 28, size=n_obj).astype(np.int64))
    g["rooms"].x, g["rooms"].pos = feats(n_rooms, False)
    g["rooms"].y = torch.from_numpy(rng.integers(0, workloads.NUM_ROOM_LABELS, size=n_rooms).astype(np.int64))
    g["objects", "objects_to_objects", "objects"].edge_index = torch.from_numpy(oo)
    g["rooms", "rooms_to_rooms", "rooms"].edge_index = torch.from_numpy(rr)
    g["objects", "objects_to_rooms", "rooms"].edge_index = torch.from_numpy(ro[::-1].copy())
    g["rooms", "rooms_to_objects", "objects"].edge_index = torch.from_numpy(ro)
    return g


def regime_batch(edge):
    rng = np.random.default_rng(4242)
    graphs = [regime_scene(rng, [0, 1, 31, 32, 33, 64, 150], hub_room=6), workloads.mp3d_like_graph(rng),
              regime_scene(rng, [65, 2, 0, 17], hub_room=0)]
    if edge:
        for g in graphs:
            compute_relative_pos(g)
    b = collate(graphs)
    n_rooms = b["rooms"].x.size(0)
    to_room = torch.bincount(b["objects", "objects_to_rooms", "rooms"].edge_index[1], minlength=n_rooms)
    n_obj = b["objects"].x.size(0)
    to_obj = torch.bincount(b["objects", "objects_to_objects", "objects"].edge_index[1], minlength=n_obj) + 1
    assert (to_room == 0).any(), "no empty room"
    assert {31, 32, 33, 64, 65, 150} <= set(to_room.tolist())
    assert int(to_obj.max()) > 140, "no object hub"
    return b


@pytest.mark.parametrize("block", ["GAT", "GAT_edge"])
@pytest.mark.parametrize("hidden,heads,concats", [
    ([128, 128], [4, 4, 4], [True, True, False]),     # BASELINE config 3
    ([64, 64], [3, 3, 3], [False, False, False]),     # the shipped MP3D shape: head mean everywhere
])
def test_hetero_gat_parity_on_degree_regimes(block, hidden, heads, concats):
    ora, net = gat_pair(block, hidden, heads, concats, seed=11)
    check_model(ora, net, regime_batch(block == "GAT_edge"))


@pytest.mark.parametrize("block", ["GAT", "GAT_edge"])
def test_gat_training_mode_parity_on_degree_regimes(block):
    training_mode_parity(block, [128, 128], [4, 4, 4], [True, True, False], regime_batch(block == "GAT_edge"))


def test_homogeneous_gat_parity_with_rooms_past_the_cache():
    """room 0 receives 40 objects, room 41 100 (plus the loops): eval logits, loss and every gradient."""
    torch.manual_seed(1)
    kw = dict(input_dim=6, output_dim=15, conv_block="GAT", GAT_hidden_dims=[24], GAT_heads=[3, 3], GAT_concats=[True, False],
              dropout=0.0)
    ora = omodels.HomogeneousNetwork(**kw)
    with torch.no_grad():
        for n_, p_ in ora.named_parameters():
            if n_.endswith(".bias"):
                p_.uniform_(-0.1, 0.1)
    net = HomogeneousNetwork(**kw)
    net.load_state_dict(ora.state_dict(), strict=True)
    net = net.to(DEV).eval()
    rng = np.random.default_rng(2)
    n = 1 + 40 + 1 + 100
    objs_a, objs_b = np.arange(1, 41), np.arange(42, 142)
    src = [objs_a, objs_b, rng.choice(objs_b, 60), rng.choice(objs_a, 30)]
    dst = [np.zeros(40, np.int64), np.full(100, 41), rng.choice(objs_b, 60), rng.choice(objs_a, 30)]
    ei = torch.from_numpy(np.stack([np.concatenate(src), np.concatenate(dst)]).astype(np.int64))
    x = torch.from_numpy(rng.normal(size=(n, 6)).astype(np.float32))
    room_mask = torch.zeros(n, dtype=torch.bool)
    room_mask[[0, 41]] = True
    y = torch.from_numpy(rng.integers(0, 15, size=n).astype(np.int64))
    o64 = copy.deepcopy(ora).double().eval()
    ref = o64(Data(x=x.double(), edge_index=ei, room_mask=room_mask))
    out = net(Data(x=x, edge_index=ei, room_mask=room_mask, y=y).to(DEV))
    torch.testing.assert_close(out.detach().cpu().double(), ref.detach(), atol=ATOL, rtol=RTOL)
    yr = y[room_mask]
    loss_ref = o64.loss(ref, yr)
    loss_ref.backward()
    loss = net.loss(out, yr.to(DEV))
    torch.testing.assert_close(loss.detach().cpu().double(), loss_ref.detach(), atol=ATOL, rtol=RTOL)
    loss.backward()
    og = dict(o64.named_parameters())
    for name, q in net.named_parameters():
        if og[name].grad is None:
            assert q.grad is None, name
            continue
        assert q.grad is not None, name
        torch.testing.assert_close(q.grad.cpu().double(), og[name].grad, atol=ATOL, rtol=RTOL, msg=lambda m: f"{name}: {m}")
