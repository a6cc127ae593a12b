"""GPU checks of the attention export's unit entry: hmp_gat_fwd, then hmp_gat_attention on the softmax state it left.

alpha against the float64 reference (tests/_gat_attention_reference.py) at the ATOL / RTOL = 1e-5 of test_gpu_gat.py, the
project's standing fp32 bound (the forward outputs built from the same coefficients pass it at these sizes); the rows of removed
loops and dropped edges exactly 0.  top_src / top_w are a function of the exported alpha alone and are compared with its numpy
restatement bit for bit, padding included: a consistency condition between two outputs of one launch, not a tolerance.
Requesting one output gives the bits of requesting both.

Shapes: 7 x 7 nodes with explicit i -> i edges and a duplicated edge; 40 -> 5 nodes with 400 edges (mean degree 80, above the 16
lanes of a row group), one destination without an edge and one with exactly one; no edge at all; one edge whose source does not
exist.  Heads 1, 2, 4, 8 (every template class; 4 and 8 take the 16-byte store), the last (2 x 300) in the wide-head class of
the forward."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hydra_gnn_amd import _lib  # noqa: E402
from test_gpu_ops import build_plan, rand_edges  # noqa: E402
from _gat_attention_reference import attention_reference, kept_edges, top_from_alpha  # noqa: E402

ATOL, RTOL = 1e-5, 1e-5
DEV = "cuda:0"


def edges_of(shape, rng):
    """(ei int64 [2, E], n_src, n_dst, status the plan must report)"""
    if shape == "loops7":
        ei = rand_edges(rng, 20, 7, 7)
        ei[1, :4] = ei[0, :4]          # explicit i -> i edges
        ei[:, 11] = ei[:, 10]          # one duplicated edge
        return ei, 7, 7, 0
    if shape == "deg80":
        ei = rand_edges(rng, 400, 40, 5)
        ei[1] = torch.from_numpy(rng.integers(0, 3, 400))  # destinations 0..2 share the edges, 3 gets none ...
        ei[1, 123] = 4                                      # ... and 4 exactly one
        return ei, 40, 5, 0
    if shape == "empty":
        return torch.zeros(2, 0, dtype=torch.int64), 6, 6, 0
    assert shape == "dropped"
    ei = rand_edges(rng, 20, 7, 7)
    ei[1, :2] = ei[0, :2]
    ei[0, 6] = 9                       # a source that does not exist: the plan drops the edge
    return ei, 7, 7, 1


def run_attention(lib, case, k, want_alpha=True, want_top=True):
    H, E, n_loop, n_dst = case["H"], case["E"], case["n_loop"], case["n_dst"]
    alpha = torch.full((max(E + n_loop, 1), H), float("nan"), device=DEV) if want_alpha else None
    src = torch.full((max(n_dst, 1), k), -7, dtype=torch.int64, device=DEV) if want_top else None
    w = torch.full((max(n_dst, 1), k), float("nan"), device=DEV) if want_top else None
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _lib.check(lib.hmp_gat_attention(case["as"].data_ptr(), 8, case["ad"].data_ptr(), 8, ptr(case["ea"]), ptr(case["ve"]),
                                     case["ei_dev"].data_ptr() if E else None, case["plan"]["plan"], case["args"],
                                     case["smax"].data_ptr(), case["sden"].data_ptr(), ptr(alpha), k, ptr(src), ptr(w),
                                     _lib.stream_ptr()))
    cut = lambda t, n: t[:n].cpu().numpy() if t is not None else None  # noqa: E731
    return cut(alpha, E + n_loop), cut(src, n_dst), cut(w, n_dst)


@pytest.mark.parametrize("shape", ["loops7", "deg80", "empty", "dropped"])
@pytest.mark.parametrize("loops", [False, True])
@pytest.mark.parametrize("edge_dim", [0, 3])
@pytest.mark.parametrize("H,Cc", [(1, 8), (4, 16), (8, 32), (2, 300)])
def test_attention_unit(H, Cc, edge_dim, loops, shape):
    lib = _lib.require_device()
    rng = np.random.default_rng(1000 * H + 10 * edge_dim + int(loops) + len(shape))
    ei, n_src, n_dst, status = edges_of(shape, rng)
    E = ei.size(1)
    plan = build_plan(ei.to(DEV), n_src, n_dst)
    assert plan["status"] == status
    f = lambda *s: torch.from_numpy(rng.normal(0, 1, size=s).astype(np.float32))  # noqa: E731
    Cp = (Cc + 3) // 4 * 4
    h = f(n_src, H * Cp)
    a_s, a_d = f(n_src, H), f(n_dst, H)
    ea = f(max(E, 1), 3)[:E] if edge_dim else None
    ve = f(3, H) if edge_dim else None
    pad8 = lambda t: torch.cat([t, torch.zeros(t.size(0), 8 - t.size(1))], 1).contiguous().to(DEV)  # noqa: E731
    n_loop = min(n_src, n_dst) if loops else 0
    case = dict(H=H, E=E, n_loop=n_loop, n_dst=n_dst, plan=plan, ei_dev=ei.to(DEV), args=_lib.GatArgs(H, Cc, int(loops), edge_dim, 0.0, 0, 0, 0),
                ea=ea.contiguous().to(DEV) if edge_dim and E else None, ve=pad8(ve) if edge_dim else None)
    case["as"], case["ad"] = pad8(a_s), pad8(a_d)
    case["smax"], case["sden"] = torch.zeros(n_dst, 8, device=DEV), torch.zeros(n_dst, 8, device=DEV)
    ldo = (H * Cc + 3) // 4 * 4
    out = torch.zeros(n_dst, ldo, device=DEV)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _lib.check(lib.hmp_gat_fwd(h.to(DEV).data_ptr(), H * Cp, case["as"].data_ptr(), 8, case["ad"].data_ptr(), 8, ptr(case["ea"]),
                               ptr(case["ve"]), plan["plan"], case["args"], case["smax"].data_ptr(), case["sden"].data_ptr(),
                               out.data_ptr(), ldo, _lib.stream_ptr()))

    ref = attention_reference(a_s, a_d, ea, ve, ei, n_src, n_dst, loops)
    keep = kept_edges(ei, n_src, n_dst, loops).numpy()
    first = None
    for k in (1, 3, 8):
        alpha, src, w = run_attention(lib, case, k)
        assert alpha.shape == (E + n_loop, H) and src.shape == (n_dst, k) and w.shape == (n_dst, k)
        err = np.abs(alpha.astype(np.float64) - ref.numpy())
        print(f"H={H} edge_dim={edge_dim} loops={loops} {shape} k={k}: max |alpha - ref| = {err.max() if err.size else 0.0:.3e}")
        torch.testing.assert_close(torch.from_numpy(alpha).double(), ref, atol=ATOL, rtol=RTOL)
        assert (alpha[:E][~keep] == 0).all(), "a removed loop's or a dropped edge's row is not exactly 0"
        want_src, want_w = top_from_alpha(alpha, ei, n_src, n_dst, loops, k)
        assert np.array_equal(src, want_src), f"k={k}: top_src differs from the order of the exported alpha"
        assert np.array_equal(w.view(np.uint32), want_w.view(np.uint32)), f"k={k}: top_w differs from the means of the exported alpha"
        if first is None:
            first = alpha
        assert np.array_equal(alpha.view(np.uint32), first.view(np.uint32)), "alpha depends on k"
    # one output alone holds the bits it holds next to the others
    only_alpha, none_s, none_w = run_attention(lib, case, 3, want_top=False)
    assert none_s is None and none_w is None and np.array_equal(only_alpha.view(np.uint32), first.view(np.uint32))
    both = run_attention(lib, case, 3)
    none_a, only_src, only_w = run_attention(lib, case, 3, want_alpha=False)
    assert none_a is None and np.array_equal(only_src, both[1]) and np.array_equal(only_w.view(np.uint32), both[2].view(np.uint32))
    if shape == "deg80":
        deg = np.bincount(ei[1].numpy(), minlength=n_dst)
        assert deg.max() > 16 and deg[3] == 0 and deg[4] == 1
        assert (both[1][3, (1 if loops else 0):] == -1).all() and (both[2][3, (1 if loops else 0):] == 0).all()


def test_attention_refusals():
    lib = _lib.require_device()
    rng = np.random.default_rng(5)
    ei = rand_edges(rng, 10, 4, 4)
    plan = build_plan(ei.to(DEV), 4, 4)
    z = torch.zeros(4, 8, device=DEV)
    args = _lib.GatArgs(2, 8, 0, 0, 0.0, 0, 0, 0)
    for k in (0, 9, -1):
        rc = lib.hmp_gat_attention(z.data_ptr(), 8, z.data_ptr(), 8, None, None, None, plan["plan"], args, z.data_ptr(), z.data_ptr(),
                                   None, k, None, None, _lib.stream_ptr())
        assert rc == 1 and b"k = " in lib.hmp_last_error()
    rc = lib.hmp_gat_attention(z.data_ptr(), 8, z.data_ptr(), 8, None, None, None, plan["plan"], args, None, z.data_ptr(), None, 3, None,
                               None, _lib.stream_ptr())
    assert rc == 1 and b"null pointer" in lib.hmp_last_error()
