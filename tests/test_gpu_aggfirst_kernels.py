"""The aggregate-first kernels (csrc/aggfirst.hip: seg_mean_rows_kernel, seg_mean_rows_t_kernel) and the gather-add term of the
input-gradient GEMM (gemm_bf16_dx_kernel's epilogue, its Cadd fallback on the tiled kernel), driven through their unit entries on
raw CSR arrays built in numpy, against the float64 restatement in tests/_aggfirst_reference.py (itself checked on the CPU by
tests/test_aggfirst_reference.py).

Inputs are chosen so that fp32 arithmetic is exact wherever the contract allows it -- small integers (exact in bf16 too), in-degrees
that are powers of two where the reciprocal degree is an input, p = 0.5 (scale 2), activations in quarters -- so an error cannot hide
in accumulation noise; one gaussian case per kernel checks the accumulation itself.  Every bound below is derived from the
roundings the operation may make, counted beside the assert.  Every output buffer is pre-filled with 7.0 and is wider and longer
than what the call owns: columns from align4(F) on and rows past n_rows must come back untouched."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hydra_gnn_amd import _lib  # noqa: E402
from _aggfirst_reference import (ACT_ELU, ACT_NONE, ACT_RELU, dx_gather_reference, edges_with_extents, lists_from_edges,  # noqa: E402
                                 mask_factor, seg_mean_reference, transposed_terms)

DEV = "cuda:0"
FILL = 7.0
EPS32 = 2.0 ** -24  # one fp32 rounding, relative
POISON = 1e30


def align4(f):
    return (f + 3) & ~3


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def call(fn, *args):
    rc = fn(*args)
    torch.cuda.synchronize()
    return rc


def filled(rows, ld, dtype=torch.float32):
    return torch.full((rows, ld), FILL, device=DEV, dtype=dtype)


def untouched(buf, n_rows, first_free_col):
    b = buf.float().cpu().numpy()
    return bool(np.all(b[n_rows:] == FILL) and np.all(b[:n_rows, first_free_col:] == FILL))


# ================================================================================================================================
# seg_mean_rows: M[i] = (1 / max(deg_i, 1)) * sum of the listed rows of X
# ================================================================================================================================
DEGREES = (0, 1, 7, 8, 9, 17)  # the borders of the kernel's batch of 8 neighbour rows
MEAN_ROWS = (1, 4, 5, 37)
MEAN_F = (4, 6, 64, 256, 260, 306, 516)  # 260, 306: a second pass of 256 columns; 516: a third
N_SRC = 23


@functools.lru_cache(maxsize=None)
def mean_graph(n_rows):
    """CSR lists with row degrees cycling through DEGREES (rotated by n_rows: the small row counts cover all of them between
    them), repeated neighbour ids and the last source row as a neighbour"""
    rng = np.random.default_rng(100 + n_rows)
    deg = np.array([DEGREES[(i + n_rows) % len(DEGREES)] for i in range(n_rows)])
    dst = np.repeat(np.arange(n_rows), deg)
    src = rng.integers(0, N_SRC, dst.size)
    first = np.concatenate([[0], np.cumsum(deg)])[:-1]
    for i in range(n_rows):
        if deg[i] >= 2:
            src[first[i] + 1] = src[first[i]]  # the same neighbour twice
        if deg[i] >= 1:
            src[first[i] + deg[i] - 1] = N_SRC - 1 if i % 2 == 0 else src[first[i] + deg[i] - 1]
    rowptr, col, _, _, _ = lists_from_edges(src, dst, N_SRC, n_rows)
    assert np.array_equal(np.diff(rowptr), deg) and (col == N_SRC - 1).any()
    if n_rows >= len(DEGREES):
        assert any(len(set(col[rowptr[i]:rowptr[i + 1]].tolist())) < deg[i] for i in range(n_rows))  # repeated neighbour ids
    return rowptr, col, deg


def mean_layouts(F):
    """how the rows of X lie in memory -> (pitch, element offset of the base).  vec: whole aligned 4-vectors (the vector path);
    the element path three ways: odd (pitch F + 1), offset (the base one element off), packed (F % 4 != 0 at pitch F: the 306-d
    input features)"""
    out = {"vec": (align4(F) + 4, 0), "odd": (F + 1, 0), "offset": (align4(F) + 4, 1)}
    if F % 4:
        out["packed"] = (F, 0)
    return out


MEAN_CASES = [(F, lay) for F in MEAN_F for lay in mean_layouts(F)]


def run_mean(F, layout, x_bf16, n_rows, gaussian=False):
    lib = _lib.require_device()
    ldx, off = mean_layouts(F)[layout]
    assert layout == "vec" or ldx % 4 != 0 or off % 4 != 0
    rowptr, col, deg = mean_graph(n_rows)
    rng = np.random.default_rng(F * 7 + n_rows)
    # finite values in the pad columns too: the vector path reads them, nothing may depend on them
    xv = rng.normal(size=(N_SRC, ldx)).astype(np.float32) if gaussian else rng.integers(-8, 9, (N_SRC, ldx)).astype(np.float32)
    flat = torch.zeros(N_SRC * ldx + off, device=DEV, dtype=torch.bfloat16 if x_bf16 else torch.float32)
    flat[off:] = dev(xv).reshape(-1).to(flat.dtype)
    xval = flat[off:].float().cpu().numpy().reshape(N_SRC, ldx)  # what the kernel reads (bf16: the rounded values)
    if not gaussian:
        assert np.array_equal(xval, xv)  # small integers are exact in bf16
    ldm = align4(F) + (8 if x_bf16 else 4)
    m = filled(n_rows + 3, ldm)
    d_rowptr, d_col = dev(rowptr), dev(col)  # (named: they must outlive the call)
    rc = call(lib.hmp_seg_mean_rows, flat.data_ptr() + off * flat.element_size(), ldx, int(x_bf16), F, d_rowptr.data_ptr(),
              d_col.data_ptr(), n_rows, m.data_ptr(), ldm, _lib.stream_ptr())
    _lib.check(rc)
    got = m.cpu().numpy()
    assert untouched(m, n_rows, align4(F)), (F, layout, n_rows)
    return got[:n_rows, :F].astype(np.float64), xval[:, :F].astype(np.float64), rowptr, col, deg


@pytest.mark.parametrize("x_bf16", [0, 1], ids=["x32", "x16"])
@pytest.mark.parametrize("F,layout", MEAN_CASES, ids=[f"F{F}-{lay}" for F, lay in MEAN_CASES])
def test_segment_mean_of_rows(F, layout, x_bf16):
    seen = set()
    for n_rows in MEAN_ROWS:
        got, x, rowptr, col, deg = run_mean(F, layout, x_bf16, n_rows)
        seen |= set(deg.tolist())
        ref = seg_mean_reference(x, rowptr, col)
        # integer sums of at most 17 * 8 are exact in fp32; then the reciprocal of the degree (one rounding) and the product (one
        # rounding): 2 * 2^-24, with a factor 2 of margin
        assert np.all(np.abs(got - ref) <= 2.0 ** -22 * np.abs(ref)), (n_rows, float(np.abs(got - ref).max()))
        exact = np.isin(deg, (0, 1, 8))  # reciprocal 1 or 1/8: no rounding at all
        assert np.array_equal(got[exact], ref[exact]), n_rows
        if n_rows >= len(DEGREES):
            assert set(deg.tolist()) == set(DEGREES)
    assert seen == set(DEGREES)  # every degree appeared at this F and layout


@pytest.mark.parametrize("layout", ["vec", "odd"])
def test_segment_mean_of_rows_gaussian(layout):
    got, x, rowptr, col, deg = run_mean(260, layout, 0, 37, gaussian=True)
    ref = seg_mean_reference(x, rowptr, col)
    terms = seg_mean_reference(np.abs(x), rowptr, col)  # sum |x_j| / deg
    # deg - 1 additions, each within 2^-24 of a partial sum <= sum |x_j|; the reciprocal; the product
    bound = (deg[:, None] + 2) * EPS32 * terms
    assert np.all(np.abs(got - ref) <= bound), float((np.abs(got - ref) - bound).max())
    assert np.abs(got - ref).max() > 0  # the data did exercise rounding


# ================================================================================================================================
# seg_mean_rows_t: G[j] = factor(H[j]) . sum over the CSC row of dM[t_col[k]] * degf[t_col[k]]
# ================================================================================================================================
T_ROWS = (1, 15, 16, 17, 67)  # 4 rows per wavefront, 16 per block: the row tail of a wave and the block tail
T_F = (4, 64, 256, 260, 512)
EXTENTS = (0, 1, 2, 5)
H_VALUES = np.array([0.0, -0.0, -0.75, -0.5, -0.25, 0.5, 1.0, 1.5], dtype=np.float32)  # quarters: exact in bf16, > -1 (elu)


@functools.lru_cache(maxsize=None)
def t_graph(n_rows, pow2=True):
    """CSC lists whose extents walk EXTENTS through every position of a group of four rows (group g, position q: EXTENTS[(q + g) %
    4]: the first group starts with an empty row); power-of-two in-degrees; three destination rows without edges whose degf is
    poison"""
    shift = 3 if n_rows == 1 else 0  # a single row gets the longest extent
    ext = np.array([EXTENTS[(j % 4 + j // 4 + shift) % 4] for j in range(n_rows)])
    rng = np.random.default_rng(200 + n_rows)
    src, dst = edges_with_extents(ext, 9, rng)
    if not pow2:
        dst = rng.integers(0, 9, src.size)
    n_dst = int(dst.max()) + 1 + 3
    _, _, t_rowptr, t_col, degf = lists_from_edges(src, dst, n_rows, n_dst)
    deg = np.bincount(dst, minlength=n_dst)
    degf = degf.copy()
    degf[deg == 0] = POISON
    assert np.array_equal(np.diff(t_rowptr), ext) and (deg[-3:] == 0).all()
    if n_rows >= 16:
        for q in range(4):
            assert set(ext[q::4].tolist()) == set(EXTENTS)  # every extent in every position
    if shift == 0:
        assert ext[0] == 0
    return t_rowptr, t_col, degf, ext


@functools.lru_cache(maxsize=None)
def t_inputs(n_rows, F):
    t_rowptr, t_col, degf, ext = t_graph(n_rows)
    rng = np.random.default_rng(n_rows * 1000 + F)
    lddm = align4(F) + 4
    dm = rng.integers(-8, 9, (degf.size, lddm)).astype(np.float32)
    h = rng.choice(H_VALUES, size=(n_rows, align4(F) + 8))
    h[0, :4] = [0.0, -0.0, -0.5, 1.0]
    terms = transposed_terms(dm[:, :F], t_rowptr, t_col, degf)
    return dm, h, terms


def h_tensor(h, kind):
    if kind == "none":
        return None
    t = dev(h).to(torch.bfloat16 if kind == "h16" else torch.float32)
    assert np.array_equal(np.signbit(t.float().cpu().numpy()), np.signbit(h))  # -0.0 survives
    return t


def run_t(n_rows, F, h_kind, g_kind, act, drop_on, ldg=None, graph=None, dm=None):
    """-> (G [n_rows + 2, ldg] float64 as stored, ldg)"""
    lib = _lib.require_device()
    t_rowptr, t_col, degf, _ = graph if graph is not None else t_graph(n_rows)
    if dm is None:
        dm = t_inputs(n_rows, F)[0]
    h = h_tensor(t_inputs(n_rows, F)[1] if h_kind != "none" else None, h_kind)
    g_bf16 = g_kind == "g16"
    ldg = ldg if ldg is not None else F + (8 if g_bf16 else 4)
    g = filled(n_rows + 2, ldg, torch.bfloat16 if g_bf16 else torch.float32)
    d_dm, d_rowptr, d_col, d_degf = dev(dm), dev(t_rowptr), dev(t_col), dev(degf)  # (named: they must outlive the call)
    rc = call(lib.hmp_seg_mean_rows_t, d_dm.data_ptr(), dm.shape[1], F, d_rowptr.data_ptr(), d_col.data_ptr(),
              d_degf.data_ptr(), n_rows, h.data_ptr() if h is not None else None, h.shape[1] if h is not None else 0,
              int(h_kind == "h16"), act, int(drop_on), 2.0 if drop_on else 1.0, g.data_ptr(), ldg, int(g_bf16), _lib.stream_ptr())
    _lib.check(rc)
    return g.float().cpu().numpy().astype(np.float64)


T_MASKS = [("none", ACT_NONE, 0)] + [(hk, act, d) for hk in ("h32", "h16") for act in (ACT_NONE, ACT_RELU, ACT_ELU) for d in (0, 1)]


@pytest.mark.parametrize("g_kind", ["g32", "g16"])
@pytest.mark.parametrize("h_kind,act,drop_on", T_MASKS, ids=[f"{hk}-act{a}-drop{d}" for hk, a, d in T_MASKS])
def test_transposed_segment_mean_with_the_mask(h_kind, act, drop_on, g_kind):
    """template variants: (h32 | none, g32) <false, false>, (h16, g32) <true, false>, (h32 | none, g16) <false, true>, (h16, g16)
    <true, true>"""
    scale = 2.0 if drop_on else 1.0
    for n_rows in T_ROWS:
        for F in T_F:
            _, h, (s, _) = t_inputs(n_rows, F)
            ref = s if h_kind == "none" else mask_factor(h[:, :F], act, bool(drop_on), scale) * s
            got = run_t(n_rows, F, h_kind, g_kind, act, drop_on)
            ldg = got.shape[1]
            assert np.all(got[n_rows:] == FILL) and np.all(got[:n_rows, F:] == FILL), (n_rows, F)
            out = got[:n_rows, :F]
            if g_kind == "g32":
                # integers times powers of two, summed, times a factor in quarters: every fp32 operation is exact, so the
                # contract's 2^-22 (two roundings with margin) is met with nothing to spare
                assert np.all(np.abs(out - ref) <= 2.0 ** -22 * np.abs(ref)), (n_rows, F, float(np.abs(out - ref).max()))
            else:
                # the exact fp32 value rounded once to bf16: half an ulp = 2^-9 relative, bound 2^-8
                assert np.all(np.abs(out - ref) <= 2.0 ** -8 * np.abs(ref)), (n_rows, F, float(np.abs(out - ref).max()))
            assert ldg >= F + 4
    if h_kind != "none":
        # the signed zeros did what the contract says at the four leading elements of H: +0.0, -0.0, -0.5, 1.0
        f = mask_factor(np.array([0.0, -0.0, -0.5, 1.0], dtype=np.float32), act, bool(drop_on), scale)
        want = {(ACT_NONE, 0): [1, 1, 1, 1], (ACT_RELU, 0): [0, 0, 0, 1], (ACT_ELU, 0): [1, 1, 0.5, 1], (ACT_NONE, 1): [2, 0, 2, 2],
                (ACT_RELU, 1): [0, 0, 0, 2], (ACT_ELU, 1): [2, 0, 1.5, 2]}[(act, drop_on)]
        assert f.tolist() == want


def test_transposed_segment_mean_never_reads_degf_of_unreferenced_rows():
    """the same call with the poison replaced by 0.5 gives the same bits"""
    n_rows, F = 67, 260
    t_rowptr, t_col, degf, ext = t_graph(n_rows)
    assert (degf == POISON).sum() == 3
    calm = np.where(degf == POISON, np.float32(0.5), degf).astype(np.float32)
    a = run_t(n_rows, F, "none", "g32", ACT_NONE, 0)
    b = run_t(n_rows, F, "none", "g32", ACT_NONE, 0, graph=(t_rowptr, t_col, calm, ext))
    assert np.array_equal(a, b) and np.isfinite(a).all()


def test_transposed_segment_mean_gaussian():
    n_rows, F = 67, 260
    graph = t_graph(n_rows, pow2=False)
    t_rowptr, t_col, degf, ext = graph
    deg = np.bincount(t_col)
    assert any(int(d) & (int(d) - 1) for d in deg)  # in-degrees whose reciprocal does round
    rng = np.random.default_rng(9)
    dm = rng.normal(size=(degf.size, F + 4)).astype(np.float32)
    ref, absum = transposed_terms(dm[:, :F], t_rowptr, t_col, degf)
    got = run_t(n_rows, F, "none", "g32", ACT_NONE, 0, graph=graph, dm=dm)[:n_rows, :F]
    # per edge one product (2^-24 of the term, fused or not), ext - 1 additions each within 2^-24 of a partial sum <= sum |terms|
    bound = (ext[:, None] + 2) * EPS32 * absum
    assert np.all(np.abs(got - ref) <= bound), float((np.abs(got - ref) - bound).max())
    assert np.all(got[ext == 0] == 0)


@pytest.mark.parametrize("h_kind,act,drop_on", [("none", ACT_NONE, 0), ("h32", ACT_ELU, 1), ("h16", ACT_RELU, 1)])
@pytest.mark.parametrize("F,ldg", [(306, 306), (306, 307), (6, 7), (4, 5)])
def test_transposed_segment_mean_into_rows_that_are_not_whole_vectors(F, ldg, h_kind, act, drop_on):
    """fp32 G at a pitch that is no multiple of 4 -- the caller's input-gradient rows, 306 floats at pitch 306 (the layer-0
    objects of a one-layer net) -- takes exactly F elements per row: the neighbouring row's first elements and the spare column
    stay as they were"""
    scale = 2.0 if drop_on else 1.0
    for n_rows in (1, 17, 67):
        t_rowptr, t_col, degf, _ = t_graph(n_rows)
        rng = np.random.default_rng(F + n_rows)
        dm = rng.integers(-8, 9, (degf.size, align4(F) + 4)).astype(np.float32)
        s, _ = transposed_terms(dm[:, :F], t_rowptr, t_col, degf)
        got = None
        if h_kind == "none":
            ref = s
            got = run_t(n_rows, F, "none", "g32", act, drop_on, ldg=ldg, dm=dm)
        else:
            lib = _lib.require_device()
            h = np.random.default_rng(5).choice(H_VALUES, size=(n_rows, align4(F) + 8))
            ref = mask_factor(h[:, :F], act, bool(drop_on), scale) * s
            ht = h_tensor(h, h_kind)
            g = filled(n_rows + 2, ldg)
            d_dm, d_rowptr, d_col, d_degf = dev(dm), dev(t_rowptr), dev(t_col), dev(degf)
            _lib.check(call(lib.hmp_seg_mean_rows_t, d_dm.data_ptr(), dm.shape[1], F, d_rowptr.data_ptr(), d_col.data_ptr(),
                            d_degf.data_ptr(), n_rows, ht.data_ptr(), ht.shape[1], int(h_kind == "h16"), act, drop_on, scale,
                            g.data_ptr(), ldg, 0, _lib.stream_ptr()))
            got = g.cpu().numpy().astype(np.float64)
        assert np.all(got[n_rows:] == FILL) and np.all(got[:n_rows, F:] == FILL), n_rows
        assert np.array_equal(got[:n_rows, :F], ref), n_rows  # exact arithmetic (see above)


# ================================================================================================================================
# hmp_gemm_bf16_dx_gather: G = factor(H) . (dZ W + transposed sum), fused into the weight-stationary kernel or scratch + Cadd
# ================================================================================================================================
DX_M = 32768 + 37  # the smallest M the weight-stationary kernel takes, with a ragged last 64-row tile
DX_DST = 300
DX_TOL = 8e-3      # tests/test_gpu_ops.py::test_bf16_input_gradient_weight_stationary_kernel: bf16 output, denominator clamped at 1


@functools.lru_cache(maxsize=None)
def dx_graph():
    ext = np.array([EXTENTS[(j % 4 + j // 4 + 1) % 4] for j in range(DX_M)])
    assert ext[0] > 0 and ext[-1] > 0
    src, dst = edges_with_extents(ext, DX_DST, np.random.default_rng(77))
    _, _, t_rowptr, t_col, degf = lists_from_edges(src, dst, DX_M, DX_DST)
    deg = np.bincount(dst, minlength=DX_DST)
    assert deg.min() >= 1 and np.array_equal(np.diff(t_rowptr), ext)
    return t_rowptr, t_col, degf, deg


@functools.lru_cache(maxsize=None)
def dx_gather(N):
    """g_rows = in-degree * an integer of magnitude 8..12: ONE edge contributes +-8..12 to an element, exactly; and the float64 term
    with its two arithmetic mutants (an edge dropped, degf ignored)"""
    t_rowptr, t_col, degf, deg = dx_graph()
    rng = np.random.default_rng(N)
    g_ld = N + 4
    v = rng.integers(8, 13, (DX_DST, g_ld)) * rng.choice([-1, 1], size=(DX_DST, g_ld))
    g_rows = (v * deg[:, None]).astype(np.float32)
    term, _ = transposed_terms(g_rows[:, :N], t_rowptr, t_col, degf)
    k = t_rowptr[DX_M // 2 + 1] - 1  # the last entry of a middle row
    j = int(np.searchsorted(t_rowptr, k, side="right") - 1)
    dropped = term.copy()
    dropped[j] -= g_rows[t_col[k], :N].astype(np.float64) * float(degf[t_col[k]])
    no_degf, _ = transposed_terms(g_rows[:, :N], t_rowptr, t_col, np.ones_like(degf))
    return g_rows, term, dropped, no_degf


def dx_err(got, ref):
    return float((np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)).max())


@pytest.mark.parametrize("mask", ["relu_drop", "none"])
@pytest.mark.parametrize("N,K,split", [(128, 256, 0), (256, 256, 0), (128, 512, 256), (256, 512, 0), (256, 512, 256)])
def test_input_gradient_gemm_with_the_gather_add_term(monkeypatch, N, K, split, mask):
    lib = _lib.require_device()
    M, pad = DX_M, 8
    t_rowptr, t_col, degf, _ = dx_graph()
    g_rows, term, dropped, no_degf = dx_gather(N)
    g_ld = g_rows.shape[1]
    assert g_ld == N + 4
    gen = torch.Generator(device=DEV).manual_seed(N + K + split)
    k1 = split if split else K
    A1 = (torch.randn(M, k1 + pad, device=DEV, generator=gen) * 0.5).to(torch.bfloat16)
    A2 = (torch.randn(M, (K - k1) + pad, device=DEV, generator=gen) * 0.5).to(torch.bfloat16) if split else None
    W = torch.randn(K, N + 4, device=DEV, generator=gen) * 0.1
    act, drop_on, scale = (ACT_RELU, 1, 2.0) if mask == "relu_drop" else (ACT_NONE, 0, 1.0)
    H = h = None
    if mask != "none":
        H = torch.randn(M, N + pad, device=DEV, generator=gen).to(torch.bfloat16)
        H = torch.where(torch.rand(M, N + pad, device=DEV, generator=gen) < 0.5, torch.tensor(-0.0, device=DEV, dtype=torch.bfloat16), H)
        assert int((H.view(torch.int16) == -32768).sum()) > M  # the -0 pattern survives
        h = H.float().cpu().numpy()
    Afull = torch.cat([A1[:, :k1], A2[:, : K - k1]], dim=1) if split else A1[:, :K]
    prod = (Afull.double() @ W[:, :N].to(torch.bfloat16).double()).cpu().numpy()  # float64 on the rounded operands
    ref = dx_gather_reference(prod, term, h, act, bool(drop_on), scale)
    # ---- the case is sized so that the gather term dominates the bound: one edge's contribution (>= 8) is at least ten times the
    # tolerance at any element, and three wrong kernels would fail the assert below (reference against reference, on the CPU)
    # (before the mask: a factor of 2 scales the contribution and the tolerance alike, a factor of 0 hides the element from any test)
    assert 8.0 >= 10 * DX_TOL * max(float(np.abs(prod + term).max()), 1.0)
    assert dx_err(dx_gather_reference(prod, dropped, h, act, bool(drop_on), scale), ref) >= DX_TOL  # one edge dropped
    assert dx_err(dx_gather_reference(prod, no_degf, h, act, bool(drop_on), scale), ref) >= DX_TOL  # degf ignored
    if h is not None:
        f = mask_factor(h[:, :N], act, bool(drop_on), scale)
        assert dx_err(f * prod + term, ref) >= DX_TOL  # the mask applied before the add (without a mask there is no such mistake)
    d_rowptr, d_col, d_degf, d_rows = dev(t_rowptr), dev(t_col), dev(degf), dev(g_rows)
    outs = {}
    for mode in (None, "0"):  # None: fused into the weight-stationary kernel's epilogue; 0: scratch + Cadd on the tiled kernel
        if mode is None:
            monkeypatch.delenv("HMP_GEMM_DX", raising=False)
        else:
            monkeypatch.setenv("HMP_GEMM_DX", mode)
        G = filled(M, N + pad, torch.bfloat16)
        scratch = filled(M, g_ld)
        _lib.check(call(lib.hmp_gemm_bf16_dx_gather, A1.data_ptr(), k1 + pad, A2.data_ptr() if split else None,
                        (K - k1) + pad if split else 0, split, W.data_ptr(), N + 4, H.data_ptr() if H is not None else None, N + pad, act,
                        drop_on, scale, G.data_ptr(), N + pad, M, N, K, d_rowptr.data_ptr(), d_col.data_ptr(), d_degf.data_ptr(),
                        d_rows.data_ptr(), g_ld, scratch.data_ptr(), _lib.stream_ptr()))
        sc = scratch.cpu().numpy()
        if mode is None:
            assert np.all(sc == FILL)  # fused: the term was never materialised
        else:
            assert np.array_equal(sc[:, :N].astype(np.float64), term)  # exact integers
        got = G[:, :N].float().cpu().numpy().astype(np.float64)
        err = dx_err(got, ref)
        # bf16 output: half an ulp of 2^-8 relative = 3.9e-3, plus the fp32 accumulation of K products (the existing dx bound)
        assert err < DX_TOL, (mode, err)
        assert torch.all(G[:, N:] == FILL)
        outs[mode] = got
    monkeypatch.delenv("HMP_GEMM_DX", raising=False)
    # same products on the same matrix pipe; the term joins the sum first (Cadd) or last (epilogue): a last-bit difference in the
    # fp32 sum can move a bf16 rounding -- a handful, as the existing dx test allows
    assert int((outs[None] != outs["0"]).sum()) <= M * N // 2000


# ================================================================================================================================
# refusals: an error, and nothing launched
# ================================================================================================================================
def test_arguments_the_launchers_refuse(monkeypatch):
    lib = _lib.require_device()
    n, F = 5, 8
    x = filled(8, F)
    rowptr = torch.zeros(DX_M + 1, device=DEV, dtype=torch.int32)  # no entries: a launch that slipped through reads no row
    col = torch.zeros(4, device=DEV, dtype=torch.int32)
    degf = torch.ones(8, device=DEV)
    out = filled(8, 16)
    args_m = lambda ldm: (x.data_ptr(), F, 0, F, rowptr.data_ptr(), col.data_ptr(), n, out.data_ptr(), ldm, _lib.stream_ptr())  # noqa: E731
    assert call(lib.hmp_seg_mean_rows, *args_m(16)) == 0
    assert torch.all(out[:n, :F] == 0) and untouched(out, n, F)
    out.fill_(FILL)
    assert call(lib.hmp_seg_mean_rows, *args_m(F + 1)) != 0  # output pitch % 4 != 0
    assert b"seg_mean_rows" in lib.hmp_last_error()
    args_t = lambda Ft, lddm, ldg, g16: (x.data_ptr(), lddm, Ft, rowptr.data_ptr(), col.data_ptr(), degf.data_ptr(), n, None, 0, 0, 0, 0, 1.0,  # noqa: E731
                                         out.data_ptr(), ldg, g16, _lib.stream_ptr())
    assert call(lib.hmp_seg_mean_rows_t, *args_t(6, 8, 8, 0)) != 0  # F % 4 != 0 into rows of whole vectors
    assert b"seg_mean_rows_t" in lib.hmp_last_error()
    assert call(lib.hmp_seg_mean_rows_t, *args_t(4, 7, 8, 0)) != 0  # dM pitch % 4 != 0
    assert call(lib.hmp_seg_mean_rows_t, *args_t(4, 8, 6, 1)) != 0  # bf16 G has no element-wise store
    assert call(lib.hmp_seg_mean_rows_t, *args_t(8, 8, 6, 0)) != 0  # G pitch below F
    assert torch.all(out == FILL)
    # the dx entry with a gather pitch that is no multiple of 4: the weight-stationary kernel must not fuse it, and the fallback's
    # launcher refuses the same pitch -- an error, nothing launched
    monkeypatch.delenv("HMP_GEMM_DX", raising=False)
    M, N, K, g_ld = DX_M, 128, 256, 128 + 5
    A = torch.zeros(M, K, device=DEV, dtype=torch.bfloat16)
    W = torch.zeros(K, N, device=DEV)
    G = filled(M, N, torch.bfloat16)
    rows = torch.zeros(4, g_ld, device=DEV)
    scratch = filled(M, g_ld)
    rc = call(lib.hmp_gemm_bf16_dx_gather, A.data_ptr(), K, None, 0, 0, W.data_ptr(), N, None, 0, 0, 0, 1.0, G.data_ptr(), N, M, N, K,
              rowptr.data_ptr(), col.data_ptr(), degf.data_ptr(), rows.data_ptr(), g_ld, scratch.data_ptr(), _lib.stream_ptr())
    assert rc != 0 and b"seg_mean_rows_t" in lib.hmp_last_error()
    assert torch.all(G == FILL) and torch.all(scratch == FILL)
