"""K3 (csrc/gat.hip) with heads wider than 256 channels: the 64-lane row group whose lanes own two 4-channel slices per head
(channels 4g.. and 256+4g..), for 256 < align4(C) <= 512 and up to 4 heads.

hmp_gat_fwd + hmp_gat_bwd through test_gpu_gat_kernels.run_unit: float64 reference (gat_reference_full), every output buffer
NaN before the call (each documented element written, everything else still NaN afterwards), two identical calls equal bit
for bit.  The graphs are that file's degree-regime graphs -- rows of 0, 1, UB-1, UB, UB+1, 31, 32, 33, 64 and 65 slots, a
destination hub, a source hub, removed self loops, duplicate edges -- built for the fetch-batch depth the wide class uses
(4 while heads x slices <= 4, else 2).

Shapes: one channel into the second slice (257, C % 4 != 0: element-wise gradient loads), 258, 306 (a `pre_mp` over the MP3D
features: lanes 0..12 hold a second slice), 512 (every lane holds both), 2 x 260, 3 x 306 (heads-class 4 with a dead head,
edge attributes of width 3, attention dropout 0.5), 4 x 264, 4 x 512 (the largest footprint); 256-channel controls on the old
class.  Strided / 4-byte-offset gradients make C % 4 == 0 take the element-wise path too.  5 x 257 and 1 x 513 are refused
(HMP_E_ARG) before anything is launched.

Tolerance: run_unit's 1e-5 (atol + rtol) against float64, the figure of test_gpu_gat_kernels.py.  Every case meets it on an
MI355X, the 512-channel dot products on the hub rows of 4 x 512 included, so no wider bound is derived or used.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hydra_gnn_amd import _lib  # noqa: E402
from test_gpu_gat_kernels import (DEV, HMAX, NAN, align4, check_regimes, dispatch_class, regime_graph,  # noqa: E402
                                  run_unit)
from test_gpu_ops import build_plan  # noqa: E402

HMP_E_ARG = 1


def wide_class(H, C):
    """(heads-class, row-group width, slices per lane) of gat.hip dispatch(); None where it refuses"""
    hm, gs = dispatch_class(H, C)
    lanes = align4(C) // 4
    if lanes <= 64:
        return hm, gs, 1
    if lanes <= 128 and H <= 4:
        return hm, 64, 2
    return None


def batch_depth(H, C):
    hm, _, r = wide_class(H, C)
    return 4 if hm * r <= 4 else 2


def wide_case(seed, H, C, geometry, loops, budget=4_500_000):
    """test_gpu_gat_kernels.regime_case with the fetch-batch depth of the class that H x C really runs"""
    slots = min(7000, budget // (H * C))
    hub, fan = min(3000, int(0.45 * slots)), min(1100, int(0.2 * slots))
    n = fan + 24
    n_src, n_dst = {"eq": (n, n), "src<dst": (n - 8, n), "src>dst": (n + 8, n)}[geometry]
    ub = batch_depth(H, C)
    ei = regime_graph(seed, n_src, n_dst, loops, ub, hub, fan)
    check_regimes(ei, n_src, n_dst, loops, ub, hub, fan)
    return ei, n_src, n_dst


WIDE_CASES = [
    # H, C, geometry, loops, edim, p, layout
    (1, 257, "eq", 1, 0, 0.0, "dense"),
    (1, 258, "src<dst", 0, 0, 0.0, "strided"),
    (1, 306, "eq", 1, 0, 0.0, "dense"),
    (1, 306, "src<dst", 0, 0, 0.0, "dense"),     # pre_mp: no self loops
    (1, 306, "src>dst", 1, 0, 0.0, "strided"),
    (1, 306, "eq", 0, 2, 0.0, "offset"),
    (1, 512, "eq", 1, 0, 0.0, "dense"),
    (1, 512, "src>dst", 0, 0, 0.0, "offset"),
    (2, 260, "src>dst", 1, 2, 0.0, "dense"),
    (3, 306, "eq", 1, 3, 0.5, "dense"),
    (3, 306, "src<dst", 0, 3, 0.5, "strided"),
    (4, 264, "eq", 0, 0, 0.0, "strided"),
    (4, 512, "eq", 1, 0, 0.0, "dense"),
    (4, 512, "src<dst", 0, 1, 0.0, "offset"),
    (4, 512, "src>dst", 1, 0, 0.25, "strided"),
    (1, 256, "eq", 1, 0, 0.0, "dense"),          # boundary controls: the one-slice class
    (4, 256, "eq", 1, 0, 0.0, "dense"),
]


def test_wide_cases_reach_every_wide_instantiation():
    reached = {wide_class(c[0], c[1]) for c in WIDE_CASES}
    assert {(1, 64, 2), (2, 64, 2), (4, 64, 2), (1, 64, 1), (4, 64, 1)} == reached
    for shape in [(1, 306), (4, 512)]:
        mine = [c for c in WIDE_CASES if (c[0], c[1]) == shape]
        assert {c[2] for c in mine} == {"eq", "src<dst", "src>dst"} and {c[3] for c in mine} == {0, 1}
    assert {c[6] for c in WIDE_CASES if c[1] == 512} == {"dense", "offset", "strided"}
    assert wide_class(5, 257) is None and wide_class(1, 513) is None and wide_class(8, 256) == (8, 64, 1)


@pytest.mark.parametrize("H,Cc,geometry,loops,edim,p,layout", WIDE_CASES,
                         ids=[f"H{c[0]}-C{c[1]}-{c[2]}-loops{c[3]}-e{c[4]}-p{c[5]}-{c[6]}" for c in WIDE_CASES])
def test_gat_unit_wide_heads_on_degree_regimes(H, Cc, geometry, loops, edim, p, layout):
    ei, n_src, n_dst = wide_case(H * 1000 + Cc, H, Cc, geometry, loops)
    r = run_unit(H, Cc, ei, n_src, n_dst, loops, edim=edim, p=p, layout=layout, seed=H + Cc)
    if p > 0:
        assert 0 < r["keep"][:, :H].float().mean() < 1


def test_gat_unit_wide_loops_only():
    """E = 0 with self_loops = 1: the loop is the only slot of every row < min(n_src, n_dst)"""
    run_unit(2, 306, torch.zeros(2, 0, dtype=torch.int64), 5, 7, 1, edim=3, layout="strided")
    run_unit(1, 512, torch.zeros(2, 0, dtype=torch.int64), 7, 5, 1, p=0.5)


@pytest.mark.parametrize("H,Cc,words", [(5, 257, (b"512", b"256")), (8, 512, (b"512", b"256")), (1, 513, (b"512", b"256"))])
def test_gat_unit_refuses_what_no_class_covers(H, Cc, words):
    """more than 4 heads above 256 channels, more than 512 channels: HMP_E_ARG naming both limits, no launch (every output
    still NaN)"""
    lib = _lib.require_device()
    rng = np.random.default_rng(H + Cc)
    n, E = 9, 30
    ei = torch.from_numpy(rng.integers(0, n, size=(2, E)).astype(np.int64))
    plan = build_plan(ei.to(DEV), n, n)
    assert plan["status"] == 0
    Cp, P = align4(Cc), E + n
    h = torch.ones(n, H * Cp, device=DEV)
    a = torch.ones(n, HMAX, device=DEV)
    g = torch.ones(n, align4(H * Cc), device=DEV)
    o = dict(smax=torch.full((n, HMAX), NAN, device=DEV), sden=torch.full((n, HMAX), NAN, device=DEV),
             out=torch.full((n, align4(H * Cc)), NAN, device=DEV), alpha_drop=torch.full((P, HMAX), NAN, device=DEV),
             dlogit=torch.full((P, HMAX), NAN, device=DEV), dlogit_orig=torch.full((E, HMAX), NAN, device=DEV),
             g_h=torch.full((n, H * Cp), NAN, device=DEV), g_as=torch.full((n, HMAX), NAN, device=DEV),
             g_ad=torch.full((n, HMAX), NAN, device=DEV))
    args = _lib.GatArgs(H, Cc, 1, 0, 0.0, 1, 0, 0)
    torch.cuda.synchronize()
    rc = lib.hmp_gat_fwd(h.data_ptr(), H * Cp, a.data_ptr(), HMAX, a.data_ptr(), HMAX, None, None, plan["plan"], args,
                         o["smax"].data_ptr(), o["sden"].data_ptr(), o["out"].data_ptr(), align4(H * Cc), _lib.stream_ptr())
    msg = lib.hmp_last_error()
    assert rc == HMP_E_ARG and all(w in msg for w in words), (rc, msg)
    torch.cuda.synchronize()
    for k in ("smax", "sden", "out"):
        assert torch.isnan(o[k]).all(), f"{k}: written by a refused call"
    # a valid forward state, so that only the shape can be what the backward refuses
    o["smax"].fill_(0.0)
    o["sden"].fill_(1.0)
    rc = lib.hmp_gat_bwd(g.data_ptr(), align4(H * Cc), h.data_ptr(), H * Cp, a.data_ptr(), HMAX, a.data_ptr(), HMAX, None, None,
                         plan["plan"], args, o["smax"].data_ptr(), o["sden"].data_ptr(), o["alpha_drop"].data_ptr(),
                         o["dlogit"].data_ptr(), o["dlogit_orig"].data_ptr(), o["g_h"].data_ptr(), H * Cp, o["g_as"].data_ptr(), HMAX,
                         o["g_ad"].data_ptr(), HMAX, _lib.stream_ptr())
    msg = lib.hmp_last_error()
    assert rc == HMP_E_ARG and all(w in msg for w in words), (rc, msg)
    torch.cuda.synchronize()
    for k in ("out", "alpha_drop", "dlogit", "dlogit_orig", "g_h", "g_as", "g_ad"):
        assert torch.isnan(o[k]).all(), f"{k}: written by a refused call"
